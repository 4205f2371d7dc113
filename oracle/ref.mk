# Builds oracle/_ref/ref_probe_*: oracle/ref_probe.cpp over a checkout of the reference (REF), one binary per compile-time
# variant, because tree shape, eps, packet width and max_ray_depth are template arguments and constants there.
#   make -f ref.mk REF=/path/to/reference [WIDTHS="4 8 16"]      (default WIDTHS: what this host can run)
# Writes only into _ref/ (ignored by git).  Nothing of the reference is copied: its headers are found through -I, after
# ref_shim/, which holds our stand-ins (C++23 library pieces, stb_image.h declarations, config.hpp with -D constants).
# -ffp-contract=off and no fast-math: the same arithmetic as oracle/Makefile.  g++ 11 rejects the reference's two-argument
# operator[], hence clang.
REF     ?= ../../reference
REFCXX  ?= /opt/rocm/llvm/bin/clang++
# widths this host can run: 4 always, 8 with AVX2, 16 with AVX-512
WIDTHS  ?= 4 $(if $(shell grep -m1 -w avx2 /proc/cpuinfo),8) $(if $(shell grep -m1 -w avx512bw /proc/cpuinfo),16)
OUT     := _ref
FLAGS   := -std=c++23 -O2 -ffp-contract=off -pthread -Wno-unknown-attributes -include ref_shim/cxx23_shim.hpp -I. -Iref_shim -I$(REF)/include

# native_simd<float> width <- ISA: plain x86-64 is what the reference's own CMake file gives
ISA_4   := -march=x86-64
ISA_8   := -march=x86-64-v3
ISA_16  := -march=x86-64-v4

# name = max_depth max_leaf_size eps; keep in step with TREES / EPS of tests/test_gpu_tree_params.py and REF_TREES of __init__.py
TREE_default     := 8 64 1e-6
TREE_root_leaf   := 0 64 1e-6
TREE_d12_l8      := 12 8 1e-6
TREE_d13_l4      := 13 4 1e-6
TREE_d16_l1      := 16 1 1e-6
TREE_long_leaves := 8 1000 1e-6
TREE_eps_flt_min := 8 64 1.17549435e-38
TREE_eps_1e-9    := 8 64 1e-9
TREE_eps_1e-3    := 8 64 1e-3
TREE_eps_0.25    := 8 64 0.25
TREES   := default root_leaf d12_l8 d13_l4 d16_l1 long_leaves eps_flt_min eps_1e-9 eps_1e-3 eps_0.25

SRC     := ref_probe.cpp ref.mk $(wildcard ref_shim/*.h*) ref_shim/raytracer/config.hpp $(wildcard $(REF)/include/raytracer/*.hpp $(REF)/include/raytracer/*/*.hpp $(REF)/include/raytracer/*/*/*.hpp)
tree_defs = -DRTK_REF_TREE_DEPTH=$(word 1,$(TREE_$(1))) -DRTK_REF_TREE_LEAF=$(word 2,$(TREE_$(1))) -DRTK_REF_EPSILON=$(word 3,$(TREE_$(1)))

ALL :=
# $(1) width, $(2) max_ray_depth, $(3) tree
define VARIANT
ALL += $(OUT)/ref_probe_w$(1)_d$(2)_$(3)
$(OUT)/ref_probe_w$(1)_d$(2)_$(3): $(SRC)
	@mkdir -p $(OUT)
	$(REFCXX) $(FLAGS) $(ISA_$(1)) -DRTK_REF_MAX_RAY_DEPTH=$(2) $(call tree_defs,$(3)) ref_probe.cpp -o $$@
endef
# every tree at every width with max_ray_depth 5; the default tree also with 10, and with 1 and 16 (the ends of the API's range)
$(foreach w,$(WIDTHS),$(foreach t,$(TREES),$(eval $(call VARIANT,$(w),5,$(t)))))
$(foreach w,$(WIDTHS),$(eval $(call VARIANT,$(w),10,default)))
$(foreach w,$(WIDTHS),$(eval $(call VARIANT,$(w),1,default)))
$(foreach w,$(WIDTHS),$(eval $(call VARIANT,$(w),16,default)))

# kd_tree_accel (--scalar), leaf size 64
ALL += $(OUT)/ref_probe_scalar_d5_default
$(OUT)/ref_probe_scalar_d5_default: $(SRC)
	@mkdir -p $(OUT)
	$(REFCXX) $(FLAGS) $(ISA_4) -DRTK_REF_SCALAR -DRTK_REF_MAX_RAY_DEPTH=5 $(call tree_defs,default) ref_probe.cpp -o $@

ref: $(ALL)
clean:
	rm -rf $(OUT)
.DEFAULT_GOAL := ref
.PHONY: ref clean
