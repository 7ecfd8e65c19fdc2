// TEST-ONLY: the table builder of the partial-trace engine as a host-only shared object (build_partial_trace_build() of __graft_entry__.py):
// the ptb_* entries of partial_trace_build.hpp and nothing else.  No HIP header, no device: tests/test_partial_trace_kernels_ref_cpu.py reads
// the tables of the very cases the GPU tests run from it.
#include "partial_trace_build.hpp"
