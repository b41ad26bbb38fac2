# The reference's own harnesses, compiled UNMODIFIED against this runtime
# (drop-in check), into oracle/_ref/.  Included by parameter-server_amd/Makefile
# (ROOT, LIB, HOST_HDRS and PS_BUILD are its own).  Only where the reference tree
# exists; the binaries travel with the tree as build products, the reference
# sources never do.  They find libpsgpu.so relative to themselves (PS_LIBS'
# $ORIGIN rpath), so the tree may be copied elsewhere after the build.
REF_TESTS ?= /root/reference/tests
REF_OUT   := $(ROOT)/../oracle/_ref
DROPIN    := test_connection test_simple_app test_kv_app test_kv_app_benchmark test_kv_app_multi_workers test_my LR_ps
DROPIN_BINS := $(addprefix $(REF_OUT)/,$(DROPIN))
$(REF_OUT)/%: $(REF_TESTS)/%.cpp $(LIB)/libps.a $(LIB)/libps_main.a $(LIB)/libpsgpu.so $(HOST_HDRS)
	@mkdir -p $(dir $@)
	$(call PS_BUILD,$<,$@,-w)
# Our harnesses that include the reference's own headers (tests/harness_ref):
# the reference LR server beside ours, built from the reference tree as it lies.
REF_PIN_BINS := $(patsubst $(ROOT)/../tests/harness_ref/%.cpp,$(REF_OUT)/%,$(wildcard $(ROOT)/../tests/harness_ref/*.cpp))
$(REF_OUT)/%: $(ROOT)/../tests/harness_ref/%.cpp $(LIB)/libps.a $(LIB)/libps_main.a $(LIB)/libpsgpu.so $(HOST_HDRS)
	@mkdir -p $(dir $@)
	$(call PS_BUILD,$<,$@,-I$(REF_TESTS)/src)
dropin: $(if $(wildcard $(REF_TESTS)/test_kv_app.cpp),$(DROPIN_BINS) $(REF_PIN_BINS),)
.PHONY: dropin
