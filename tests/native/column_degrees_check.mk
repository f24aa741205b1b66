# The k_column_degrees checker the -m gpu suite runs (tests/test_gpu_constraint_degrees.py);
# built by __graft_entry__.build() like deep_inv_check, in a file of its own:
# make -C tests/native -f column_degrees_check.mk
HIPCC ?= /opt/rocm/bin/hipcc
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CSRC := $(HERE)../../zk_stark_project_amd/csrc
FLAGS := -O3 -std=c++17 --offload-arch=gfx950
DEPS := $(wildcard $(CSRC)/*.hpp) $(HERE)../../include/zkp.h

all: $(HERE)column_degrees_check

# launch_column_degrees (kernels.hip, linked directly) against a host scan of the same columns
$(HERE)column_degrees_check: $(HERE)column_degrees_check.hip $(CSRC)/kernels.hip $(DEPS)
	$(HIPCC) $(FLAGS) -x hip $(HERE)column_degrees_check.hip $(CSRC)/kernels.hip -o $@

.PHONY: all
