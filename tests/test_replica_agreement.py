"""The agreement rule of the multi-GPU resident edits without a GPU: csrc/gsr_replica.h through gsr_debug_replica_verdict.

gsr_multi_remove, _add, _duplicate, _transform and _grade run their verb on every rank's replica; each rank's counts start at -1 and
are written only by a rank that returned GSR_OK.  The rule (include/gsplat_hip.h): a refusal (not GSR_E_HIP) with no rank done keeps
the replicas as they were; GSR_OK with every rank equal to rank 0 in all counts agrees; anything else drops the geometry on every
rank.  Each case below states its expected verdict from that rule."""
import ctypes as C

import numpy as np
import pytest

GSR_OK, GSR_E_INVALID, GSR_E_HIP, GSR_E_OOM = 0, -1, -2, -6


def verdict(E, rc, counts):
    return E.replica_verdict(rc, np.asarray(counts, np.int64))


@pytest.mark.parametrize("ranks", [1, 2, 8])
@pytest.mark.parametrize("rc", [GSR_E_INVALID, GSR_E_OOM])
def test_every_rank_refused_keeps_the_refusal(pkg, rc, ranks):
    E = pkg.engine
    for k in (1, 2):
        assert verdict(E, rc, np.full((ranks, k), -1)) == E.REPLICA_KEEP_REFUSAL


@pytest.mark.parametrize("k", [1, 2])
def test_all_ok_and_equal_agree(pkg, k):
    E = pkg.engine
    for ranks in (2, 8):
        counts = np.tile(np.arange(7, 7 + k), (ranks, 1))
        assert verdict(E, GSR_OK, counts) == E.REPLICA_AGREED
    assert verdict(E, GSR_OK, np.zeros((3, k))) == E.REPLICA_AGREED                 # zero is a count like any other


def test_one_rank_that_differs_drops_all(pkg):
    E = pkg.engine
    assert verdict(E, GSR_OK, [[5], [5], [4]]) == E.REPLICA_DROP_ALL
    assert verdict(E, GSR_OK, [[4], [5], [5]]) == E.REPLICA_DROP_ALL                # rank 0 is the odd one
    # K = 2: the first counts agree, only the second differs
    assert verdict(E, GSR_OK, [[3, 10], [3, 10], [3, 11]]) == E.REPLICA_DROP_ALL
    assert verdict(E, GSR_OK, [[3, 10], [3, 11]]) == E.REPLICA_DROP_ALL
    assert verdict(E, GSR_OK, [[3, 10], [4, 10]]) == E.REPLICA_DROP_ALL


def test_a_refusal_beside_a_rank_that_is_done_drops_all(pkg):
    E = pkg.engine
    for rc in (GSR_E_INVALID, GSR_E_OOM):
        assert verdict(E, rc, [[-1], [5]]) == E.REPLICA_DROP_ALL
        assert verdict(E, rc, [[5], [-1]]) == E.REPLICA_DROP_ALL
        assert verdict(E, rc, [[0], [-1], [-1]]) == E.REPLICA_DROP_ALL              # done with a count of 0
        assert verdict(E, rc, [[-1, -1], [2, 9]]) == E.REPLICA_DROP_ALL


def test_a_hip_failure_drops_all_even_with_no_rank_done(pkg):
    """a rank may have failed behind its first write: it holds nothing any more, whatever the others did"""
    E = pkg.engine
    for ranks in (1, 2, 8):
        for k in (1, 2):
            assert verdict(E, GSR_E_HIP, np.full((ranks, k), -1)) == E.REPLICA_DROP_ALL
    assert verdict(E, GSR_E_HIP, [[5], [5]]) == E.REPLICA_DROP_ALL


def test_one_rank_ok_agrees(pkg):
    E = pkg.engine
    assert verdict(E, GSR_OK, [[42]]) == E.REPLICA_AGREED
    assert verdict(E, GSR_OK, [[1, 43]]) == E.REPLICA_AGREED


def test_bad_arguments_are_refused(pkg):
    E, L = pkg.engine, pkg.load_library()
    counts = np.zeros(4, np.int64)
    v = C.c_int(-7)
    assert L.gsr_debug_replica_verdict(GSR_OK, 2, 2, None, C.byref(v)) == GSR_E_INVALID          # no counts
    assert L.gsr_debug_replica_verdict(GSR_OK, 2, 2, counts.ctypes.data, None) == GSR_E_INVALID   # no verdict
    assert L.gsr_debug_replica_verdict(GSR_OK, 0, 2, counts.ctypes.data, C.byref(v)) == GSR_E_INVALID
    assert L.gsr_debug_replica_verdict(GSR_OK, -1, 2, counts.ctypes.data, C.byref(v)) == GSR_E_INVALID
    assert L.gsr_debug_replica_verdict(GSR_OK, 2, 0, counts.ctypes.data, C.byref(v)) == GSR_E_INVALID
    assert L.gsr_debug_replica_verdict(GSR_OK, 2, -3, counts.ctypes.data, C.byref(v)) == GSR_E_INVALID
    assert v.value == -7                                                                          # untouched
    assert L.gsr_debug_replica_verdict(GSR_OK, 2, 2, counts.ctypes.data, C.byref(v)) == GSR_OK and v.value == E.REPLICA_AGREED
    with pytest.raises(E.GsrError):
        E.replica_verdict(GSR_OK, np.zeros((0, 1), np.int64))


def test_constants_match_the_header(pkg):
    import os
    import re
    E = pkg.engine
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gsplat_hip.h")).read()
    for name, value in (("KEEP_REFUSAL", E.REPLICA_KEEP_REFUSAL), ("AGREED", E.REPLICA_AGREED), ("DROP_ALL", E.REPLICA_DROP_ALL)):
        assert re.search(r"#define GSR_REPLICA_%s\s+%d\b" % (name, value), hdr), name
    assert re.search(r"int\s+gsr_debug_replica_verdict\(int rc, int ranks, int per_rank, const int64_t\* counts, int\* verdict\);", hdr)
    assert "gsr_debug_replica_verdict" in E.C_ABI_SYMBOLS
