"""Every op that reads the WholeMemory CSR graph, on graph tensors whose storage offset is not 0 (MI355X).

The graph arrays are 1-D sub-tensor views of larger WholeMemory arrays: csr_row_ptr starts at element 3, csr_col_ptr at
element 5 (an int32 view starts 20 bytes in: neither 8- nor 16-byte aligned), the edge weights at element 7 and an edge
attribute at element 9 — odd and mutually different, so that an offset that is dropped, or taken from another array, reads
the padding or shifted data. The padding before and behind every view holds poison that cannot pass for data: a large negative
number in csr_row_ptr, an id >= n_nodes in csr_col_ptr, a huge weight, an attribute no edge has. CONTINUOUS and CHUNKED (on
this one rank a single chunk; tests/test_csr_graph_ranks_gpu.py splits the same views over several), int32 and int64 columns.

The graph is the degree ladder of tests/test_sampler_edges_gpu.py, which reaches every sampler kernel class. Every reference
is fed the unpadded arrays and every comparison is exact: the samplers against the oracle (edge ids are positions in the
view), the walks, node2vec walks and negatives against their Python restatements, the fused hop and the chain against the
two-op sequence on the same views, the chain's edge attribute against the attribute array at the returned edge ids. The check
bodies are those of tests/_csr_graph_checks.py, shared with the several-rank test."""
import numpy as np
import pytest

import _csr_graph_checks as checks
from _csr_graph_checks import Views, batch      # (the fan-outs, batch sizes and seeds of the cases are the module's constants)
from test_sampler_edges_gpu import ladder_graph

pytestmark = pytest.mark.gpu

CASES = pytest.mark.parametrize("mt,col_dtype", [("continuous", np.int32), ("continuous", np.int64), ("chunked", np.int32),
                                                 ("chunked", np.int64)])


@CASES
def test_samplers_equal_the_oracle(gpu_env, mt, col_dtype):
    v = Views(gpu_env, mt, col_dtype)
    checks.check_samplers(v, col_dtype, ladder_graph()[2].astype(col_dtype), 0)
    v.destroy()


@CASES
def test_walks_equal_the_reference(gpu_env, mt, col_dtype):
    v = Views(gpu_env, mt, col_dtype)
    checks.check_walks(v, col_dtype, batch(), 0)
    v.destroy()


@CASES
@pytest.mark.parametrize("in_order", [False, True], ids=["unsorted", "sorted"])
def test_node2vec_walks_equal_the_reference(gpu_env, mt, col_dtype, in_order):
    v = Views(gpu_env, mt, col_dtype, in_order)
    checks.check_node2vec(v, col_dtype, batch(), 0)
    v.destroy()


@CASES
@pytest.mark.parametrize("in_order", [False, True], ids=["unsorted", "sorted"])
def test_negatives_equal_the_reference(gpu_env, mt, col_dtype, in_order):
    v = Views(gpu_env, mt, col_dtype, in_order)
    checks.check_negatives(v, col_dtype, batch(), 0)
    v.destroy()


@CASES
def test_fused_hop_equals_the_two_ops(gpu_env, mt, col_dtype):
    v = Views(gpu_env, mt, col_dtype)
    checks.check_fused_hop(v, col_dtype, ladder_graph()[2], 0)
    v.destroy()


@CASES
def test_chain_equals_the_two_ops(gpu_env, mt, col_dtype):
    v = Views(gpu_env, mt, col_dtype)
    checks.check_chain(v, col_dtype, ladder_graph()[2][:101], 0)
    v.destroy()
