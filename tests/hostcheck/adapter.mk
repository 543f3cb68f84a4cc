# Host check of the VideoProcessor adapter's tile methods (hc_adapter.cpp): the rules of Makefile, plus one link rule -- the sanitized objects of the library,
# stub_hip.o, stub_hip_vp.o and VideoProcessor.o, as hc_threads links them.
#   make -f adapter.mk -j16 adapter      (AddressSanitizer + UndefinedBehaviorSanitizer only; tests/test_hostcheck_adapter_cpu.py runs it)
include $(dir $(lastword $(MAKEFILE_LIST)))Makefile

adapter: $(OUT)/asan/hc_adapter

$(OUT)/asan/hc_adapter: $(OUT)/asan/obj/hc_adapter.o $(OUT)/asan/obj/stub_hip.o $(OUT)/asan/obj/stub_hip_vp.o $(OUT)/asan/obj/VideoProcessor.o $(LIBOBJS_asan)
	$(CLANGXX) $(SAN_asan) -o $@ $^ $$(nm -u $(LIBOBJS_asan) | sed -n 's/^ *U \(__hip_fatbin_[0-9a-f]*\)$$/-Wl,--defsym,\1=hc_stub_report/p' | sort -u) -ldl -lpthread

.PHONY: adapter
