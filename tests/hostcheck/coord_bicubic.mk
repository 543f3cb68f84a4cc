# Host check of tsvpp_convert_warp_bicubic / tsvpp_convert_perspective_bicubic (hc_coord_bicubic.cpp): the rules of Makefile, plus one link rule -- the same
# sanitized objects of the library, of the VideoProcessor adapter and of the stub runtime.
#   make -f coord_bicubic.mk -j16 coord_bicubic          (AddressSanitizer + UndefinedBehaviorSanitizer only; tests/test_hostcheck_coord_bicubic_cpu.py runs it)
include $(dir $(lastword $(MAKEFILE_LIST)))Makefile

coord_bicubic: $(OUT)/asan/hc_coord_bicubic

$(OUT)/asan/hc_coord_bicubic: $(OUT)/asan/obj/hc_coord_bicubic.o $(OUT)/asan/obj/stub_hip.o $(OUT)/asan/obj/stub_hip_vp.o $(OUT)/asan/obj/VideoProcessor.o $(LIBOBJS_asan)
	$(CLANGXX) $(SAN_asan) -o $@ $^ $$(nm -u $(LIBOBJS_asan) | sed -n 's/^ *U \(__hip_fatbin_[0-9a-f]*\)$$/-Wl,--defsym,\1=hc_stub_report/p' | sort -u) -ldl -lpthread

.PHONY: coord_bicubic
