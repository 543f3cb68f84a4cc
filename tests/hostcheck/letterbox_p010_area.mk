# Host check of tsvpp_convert_letterbox_p010_area (hc_letterbox_p010_area.cpp): the rules of Makefile plus one link rule.  make -f letterbox_p010_area.mk -j16 letterbox_p010_area
include $(dir $(lastword $(MAKEFILE_LIST)))Makefile
letterbox_p010_area: $(OUT)/asan/hc_letterbox_p010_area
$(OUT)/asan/hc_letterbox_p010_area: $(OUT)/asan/obj/hc_letterbox_p010_area.o $(OUT)/asan/obj/stub_hip.o $(OUT)/asan/obj/stub_hip_vp.o $(OUT)/asan/obj/VideoProcessor.o $(LIBOBJS_asan)
	$(CLANGXX) $(SAN_asan) -o $@ $^ $$(nm -u $(LIBOBJS_asan) | sed -n 's/^ *U \(__hip_fatbin_[0-9a-f]*\)$$/-Wl,--defsym,\1=hc_stub_report/p' | sort -u) -ldl -lpthread
