# Host check of tsvpp_convert_letterbox_p010 (hc_letterbox_p010.cpp): the rules of Makefile, plus one link rule -- the same sanitized objects of the library, of the
# VideoProcessor adapter and of the stub runtime.
#   make -f letterbox_p010.mk -j16 letterbox_p010          (AddressSanitizer + UndefinedBehaviorSanitizer only; tests/test_hostcheck_letterbox_p010_cpu.py runs it)
include $(dir $(lastword $(MAKEFILE_LIST)))Makefile

letterbox_p010: $(OUT)/asan/hc_letterbox_p010

$(OUT)/asan/hc_letterbox_p010: $(OUT)/asan/obj/hc_letterbox_p010.o $(OUT)/asan/obj/stub_hip.o $(OUT)/asan/obj/stub_hip_vp.o $(OUT)/asan/obj/VideoProcessor.o $(LIBOBJS_asan)
	$(CLANGXX) $(SAN_asan) -o $@ $^ $$(nm -u $(LIBOBJS_asan) | sed -n 's/^ *U \(__hip_fatbin_[0-9a-f]*\)$$/-Wl,--defsym,\1=hc_stub_report/p' | sort -u) -ldl -lpthread

.PHONY: letterbox_p010
