# Host check of tsvpp_convert_rois_p010 (hc_rois_p010.cpp): the rules of Makefile plus one link rule.  make -f rois_p010.mk -j16 rois_p010
include $(dir $(lastword $(MAKEFILE_LIST)))Makefile
rois_p010: $(OUT)/asan/hc_rois_p010
$(OUT)/asan/hc_rois_p010: $(OUT)/asan/obj/hc_rois_p010.o $(OUT)/asan/obj/stub_hip.o $(OUT)/asan/obj/stub_hip_vp.o $(OUT)/asan/obj/VideoProcessor.o $(LIBOBJS_asan)
	$(CLANGXX) $(SAN_asan) -o $@ $^ $$(nm -u $(LIBOBJS_asan) | sed -n 's/^ *U \(__hip_fatbin_[0-9a-f]*\)$$/-Wl,--defsym,\1=hc_stub_report/p' | sort -u) -ldl -lpthread
