"""The rules of a temporal sample (include/wholememory/wholegraph_amd_ext.h section 2r) without a GPU: eligibility, the keys of
both strategies and their order live in csrc/tsample.hpp, which compiles for the host. tests/cpp/tsample_test.cpp includes that
header and csrc/pcg.hpp alone, is built here with the host compiler's address and undefined-behaviour sanitizers (and
-ffp-contract=off, as the library is) and run as a process of its own; the samples it prints are compared, bit for bit, with
tests/_tsample_ref.py, the definition restated in Python, on the temporal ladder. Nothing is loaded into this interpreter but
the oracle. Also here, because they are conditions on the definition itself: the cases the ladder must hold, the numpy form of
the draws, and the statistics of the octet, which the kernel must reproduce exactly."""
import os
import subprocess

import numpy as np
import pytest

import _tsample_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tsample") / "tsample_test")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "wholegraph_amd", "csrc"),
                         os.path.join(ROOT, "tests", "cpp", "tsample_test.cpp"), "-o", exe],
                        capture_output=True, timeout=300)
    assert cc.returncode == 0, cc.stderr.decode()[-4000:]
    return exe


def run(program, tmp_path, row_ptr, edge_time, centres, times, m, strategy, inclusive, window, seed):
    """-> offsets int32 [n + 1], edge ids int64, E_i int64 [n]"""
    numbers = [row_ptr.shape[0] - 1, edge_time.shape[0], centres.shape[0], m, ref.STRATEGIES[strategy], 1 if inclusive else 0,
               -1 if window is None else window, seed]
    numbers += list(row_ptr) + list(edge_time) + list(centres) + list(times)
    path = tmp_path / "graph.txt"
    path.write_text(" ".join(str(int(x)) for x in numbers) + "\n")
    out = subprocess.run([program, str(path)], capture_output=True, timeout=300)
    assert out.returncode == 0, (out.stdout.decode()[-2000:], out.stderr.decode()[-4000:])
    offsets, egid, counts = [0], [], []
    n_nodes = row_ptr.shape[0] - 1
    for i, line in enumerate(out.stdout.decode().splitlines()):
        head, _, rest = line.partition(":")
        assert head.split()[:2] == ["T", str(i)]
        counts.append(int(head.split()[2]))
        u = int(centres[i])
        s = int(row_ptr[u]) if 0 <= u < n_nodes else 0
        egid += [s + int(x) for x in rest.split()]
        offsets.append(len(egid))
    assert len(counts) == centres.shape[0]
    return np.array(offsets, dtype=np.int32), np.array(egid, dtype=np.int64), np.array(counts, dtype=np.int64)


def test_the_ladder_keeps_its_cases():
    """lower bounds on the REFERENCE, so that a later change of the ladder cannot empty a case"""
    print("the temporal ladder at M = %d: %s" % (ref.LADDER_M, ref.assert_ladder_measures()))


@pytest.mark.parametrize("strategy", ["uniform", "last"])
def test_samples_of_the_header_equal_the_restated_definition(program, tmp_path, strategy):
    row_ptr, _, etime, starts, ctimes = ref.temporal_ladder()
    for m, inclusive, window in ((32, True, None), (32, False, None), (33, True, 50), (1, True, None), (64, False, 0), (5, True, 50),
                                 (-1, True, None), (0, False, 50)):
        want = ref.ladder_sample(m, strategy, inclusive, window)
        got = run(program, tmp_path, row_ptr, etime, starts, ctimes, m, strategy, inclusive, window, ref.LADDER_SEED)
        what = "%s, M = %d, inclusive %s, window %s" % (strategy, m, inclusive, window)
        assert np.array_equal(got[2], want[4]), "eligible counts: " + what
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[3]), what
    # the window of the int64 extremes: position 14 is node 14 at INT64_MAX, whose row holds INT64_MIN and INT64_MAX
    none, zero = ref.ladder_sample(-1, strategy, True, None), ref.ladder_sample(-1, strategy, True, 0)
    assert none[4][14] == 65 and zero[4][14] == 22, "the distance INT64_MAX - INT64_MIN must not wrap into the window"


def test_first_centres_do_not_depend_on_the_batch(program, tmp_path):
    row_ptr, col, etime, starts, ctimes = ref.temporal_ladder()
    whole = ref.ladder_sample()
    part = ref.temporal_sample(row_ptr, col, etime, starts[:100], ctimes[:100], ref.LADDER_M, seed=ref.LADDER_SEED, draw=ref.cached_draws)
    cut = int(whole[0][100])
    assert np.array_equal(part[0], whole[0][:101]) and np.array_equal(part[3], whole[3][:cut]) and cut >= 100
    later = ref.temporal_sample(row_ptr, col, etime, starts[7:8], ctimes[7:8], ref.LADDER_M, seed=ref.LADDER_SEED, first_center=7)
    assert np.array_equal(later[3], whole[3][whole[0][7]:whole[0][8]]) and later[3].shape[0] == ref.LADDER_M


def test_numpy_draws_equal_the_stream():
    rng = np.random.default_rng(3)
    for seed, i in ((0, 0), (ref.LADDER_SEED, 7), ((1 << 64) - 1, 70000), (0x123456789ABCDEF, (1 << 31) - 3)):
        js = sorted(set([0, 1, 4999] + [int(x) for x in rng.integers(0, 1 << 20, 40)]))
        assert ref.fast_draws(seed, i, js) == ref.draws(seed, i, js), (seed, i)
    centres, times, out = ref.tiled_ladder()
    assert centres.shape[0] == 70001 and out[0].shape[0] == 70002
    whole = ref.ladder_sample()
    assert np.array_equal(out[0][:513], whole[0]) and np.array_equal(out[3][:whole[0][-1]], whole[3])
    second = slice(int(out[0][512 + 7]), int(out[0][512 + 8]))      # (the hub again, at batch position 519: other draws)
    assert not np.array_equal(out[3][second], whole[3][whole[0][7]:whole[0][8]])


def test_the_octet_is_uniform(program, tmp_path):
    """6000 centres, all the node with 8 neighbours at times 1 .. 8, at time 6, inclusive, M = 2: two of the six eligible
    positions each, uniform over the six (chi-square 1.586 over 5 degrees of freedom) and over the 15 pairs (7.92 over 14).
    The values are recorded: the kernel draws the same samples, so tests/test_tsample_gpu.py asks for exactly these."""
    row_ptr, _, etime = ref.octet()
    offsets, _, _, egid = ref.octet_sample()
    single, pairs = ref.octet_statistics(offsets, egid)
    print("the octet: chi-square %.4f over 5 dof, %.4f over 14 dof" % (single, pairs))
    assert abs(single - ref.OCTET_CHI2_SINGLE) < 1e-9 and abs(pairs - ref.OCTET_CHI2_PAIRS) < 1e-9
    assert single < 15.09 and pairs < 29.14
    got = run(program, tmp_path, row_ptr, etime, np.zeros(ref.OCTET_CENTRES, dtype=np.int64),
              np.full(ref.OCTET_CENTRES, ref.OCTET_TIME, dtype=np.int64), ref.OCTET_M, "uniform", True, None, ref.OCTET_SEED)
    assert np.array_equal(got[0], offsets) and np.array_equal(got[1], egid) and (got[2] == 6).all()
