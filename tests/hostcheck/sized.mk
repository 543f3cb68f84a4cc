# Host check of tsvpp_convert_rois_sized (hc_sized.cpp): the rules of Makefile, plus one link rule -- the same sanitized objects of the library and stub_hip.o.
#   make -f sized.mk -j16 sized          (AddressSanitizer + UndefinedBehaviorSanitizer only; tests/test_hostcheck_sized_cpu.py runs it)
include $(dir $(lastword $(MAKEFILE_LIST)))Makefile

sized: $(OUT)/asan/hc_sized

$(OUT)/asan/hc_sized: $(OUT)/asan/obj/hc_sized.o $(OUT)/asan/obj/stub_hip.o $(LIBOBJS_asan)
	$(CLANGXX) $(SAN_asan) -o $@ $^ $$(nm -u $(LIBOBJS_asan) | sed -n 's/^ *U \(__hip_fatbin_[0-9a-f]*\)$$/-Wl,--defsym,\1=hc_stub_report/p' | sort -u) -ldl -lpthread

.PHONY: sized
