# Host check of tsvpp_convert_letterbox_area (hc_letterbox_area.cpp): the rules of Makefile, plus one link rule -- the same sanitized objects of the library, of the
# VideoProcessor adapter and of the stub runtime.
#   make -f letterbox_area.mk -j16 letterbox_area          (AddressSanitizer + UndefinedBehaviorSanitizer only; tests/test_hostcheck_letterbox_area_cpu.py runs it)
include $(dir $(lastword $(MAKEFILE_LIST)))Makefile

letterbox_area: $(OUT)/asan/hc_letterbox_area

$(OUT)/asan/hc_letterbox_area: $(OUT)/asan/obj/hc_letterbox_area.o $(OUT)/asan/obj/stub_hip.o $(OUT)/asan/obj/stub_hip_vp.o $(OUT)/asan/obj/VideoProcessor.o $(LIBOBJS_asan)
	$(CLANGXX) $(SAN_asan) -o $@ $^ $$(nm -u $(LIBOBJS_asan) | sed -n 's/^ *U \(__hip_fatbin_[0-9a-f]*\)$$/-Wl,--defsym,\1=hc_stub_report/p' | sort -u) -ldl -lpthread

.PHONY: letterbox_area
