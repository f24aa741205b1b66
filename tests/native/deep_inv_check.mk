# The DEEP inverse-table checker the -m gpu suite runs (tests/test_gpu_deep_denominators.py);
# built by __graft_entry__.build() like the binaries of tests/native/Makefile, in a file of
# its own: make -C tests/native -f deep_inv_check.mk
HIPCC ?= /opt/rocm/bin/hipcc
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CSRC := $(HERE)../../zk_stark_project_amd/csrc
FLAGS := -O3 -std=c++17 --offload-arch=gfx950
DEPS := $(wildcard $(CSRC)/*.hpp) $(HERE)../../include/zkp.h

all: $(HERE)deep_inv_check

# the table of launch_deep_denominators (kernels.hip, linked directly) against Fermat inverses
$(HERE)deep_inv_check: $(HERE)deep_inv_check.hip $(CSRC)/kernels.hip $(DEPS)
	$(HIPCC) $(FLAGS) -x hip $(HERE)deep_inv_check.hip $(CSRC)/kernels.hip -o $@

.PHONY: all
