"""Chains of resident edits on the GPU: what one verb leaves behind is what the next one starts from.

gsr_move, gsr_remove and gsr_add share one re-order pipeline (csrc/gsr_resident_edit.h); these cases cross from verb to verb where the
state the pipeline carries changes kind: a storage order that goes away and comes back, a box that stops being finite, a visibility in
force while the cloud shrinks, grows past its capacity and shrinks again.

Everything is BIT-EXACT, there is no tolerance anywhere: after every step the resident planes, the cluster bounds and the storage order
are those of a fresh context that was uploaded the same host arrays on the same GPU (test_move_gpu's helpers, and its cloud of 357
splats = five full clusters and a partial one), and every case ends with a frame that is the fresh upload's frame."""
import numpy as np
import pytest

import test_move_gpu as M

N = M.N


def _new(pkg, seed, m, sh=True):
    return M._copy(pkg, M._cloud(pkg, seed, sh=sh).subset(slice(0, m)))


def _order(planes):
    return planes["order"].view(np.int32)


def _same_as_fresh(pkg, U, s, label, sh=True, vis=None):
    """U's planes against a fresh upload of s (under the visibility vis = (volumes, mask) when one is in force); returns U's planes"""
    got = M._planes(U, sh)
    if vis is None:
        want = M._fresh_planes(pkg, s, 1, sh)
    else:
        with pkg.Engine(0) as F:
            F.upload(s)
            F.set_visibility(volumes=vis[0], mask=vis[1])
            assert U.get_visibility()[1] == F.get_visibility()[1], label
            want = M._planes(F, sh)
    M._assert_same_planes(got, want, label)
    return got


def _same_last_frame(pkg, U, s, label):
    cam = M._cams(pkg, [2])[0]
    got = U.render(cam).copy()
    want = M._fresh_frames(pkg, s, [cam])[0]
    assert (want[..., 3] > 0).sum() > 100, label
    assert np.array_equal(got, want), label


# ---- 1. the storage order goes away and comes back ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sh", (True, False))
def test_the_order_switches_off_and_on(pkg, sh):
    """one splat has no order (the old permutation exists, the new one does not); 131 splats have one again"""
    A, B, Cc = M._cloud(pkg, 11, sh=sh), _new(pkg, 12, 130, sh), M._cloud(pkg, 13, sh=sh)
    gone = np.ones(N, bool)
    gone[171] = False
    with pkg.Engine(0) as U:
        U.set_option(pkg.engine.OPT_STORAGE_ORDER, 1)
        U.upload(A)
        assert not np.array_equal(_order(M._planes(U, sh)), np.arange(N)), "the upload is not ordered: the case tests nothing"
        assert U.remove(gone) == 1
        s = A.subset(~gone)
        got = _same_as_fresh(pkg, U, s, f"all but one removed (sh {sh})", sh)
        assert np.array_equal(_order(got), [0])
        s = s.concat(B)
        assert U.add(B) == 131
        assert U.get_add()["grows"] == 0 and U.get_add()["capacity"] == N
        got = _same_as_fresh(pkg, U, s, f"130 added to the one (sh {sh})", sh)
        assert not np.array_equal(_order(got), np.arange(131)), "the order did not come back"
        s = M._move(pkg, U, s, Cc.P[50:60], 50)
        _same_as_fresh(pkg, U, s, f"ten of them moved (sh {sh})", sh)
        assert U.stats()["uploads"] == 1 and U.stats()["moves"] == 1 and U.stats()["n_splats"] == 131
        _same_last_frame(pkg, U, s, f"the order off and on (sh {sh})")


# ---- 2. a non-finite position passes through ---------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_non_finite_position_passes_through(pkg):
    """a box that is not finite means upload order: the add leaves an ordered store for it, a move stays in it (the cluster bounds
    rewritten in place, no spare set), and the removal of the one splat brings the order back"""
    A, B, Cc = M._cloud(pkg, 11), _new(pkg, 12, 20), M._cloud(pkg, 13)
    B.P[7] = (np.inf, 0.0, 0.0)
    with pkg.Engine(0) as U:
        U.set_option(pkg.engine.OPT_STORAGE_ORDER, 1)
        U.upload(A)
        assert not np.array_equal(_order(M._planes(U)), np.arange(N)), "the upload is not ordered: the case tests nothing"
        s = A.concat(B)
        assert U.add(B) == N + 20
        got = _same_as_fresh(pkg, U, s, "20 added, one at infinity")
        assert np.array_equal(_order(got), np.arange(N + 20)), "a cloud with a non-finite box is not in upload order"
        s = M._move(pkg, U, s, Cc.P[100:105], 100)
        got = _same_as_fresh(pkg, U, s, "five finite ones moved beside it")
        assert np.array_equal(_order(got), np.arange(N + 20))
        gone = np.zeros(N + 20, bool)
        gone[N + 7] = True
        assert U.remove(gone) == N + 19
        s = s.subset(~gone)
        got = _same_as_fresh(pkg, U, s, "the non-finite one removed")
        assert not np.array_equal(_order(got), np.arange(N + 19)), "the order did not come back"
        _same_last_frame(pkg, U, s, "a non-finite position passed through")


# ---- 3. a visibility in force across the chain of swaps ----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sh", (True, False))
def test_visibility_state_across_the_swap_chain(pkg, sh):
    """volumes and a mask in force while the cloud shrinks, grows past its capacity, has alphas edited under the rule and loses what is
    hidden: the true alphas and the mask travel with the splats, and clearing the visibility shows the fresh upload"""
    E = pkg.engine
    A, B, Cc = M._cloud(pkg, 11, sh=sh), _new(pkg, 12, 200, sh), M._cloud(pkg, 13, sh=sh)
    volumes = [E.crop_box((0, 0, 0), 0.7)]
    hide = np.arange(N) % 3 == 0
    rng = np.random.default_rng(8)

    def visible(s, mask):
        return E.visibility_eval(E.visibility_struct(volumes, mask)[0], s.P)

    with pkg.Engine(0) as U:
        U.set_option(E.OPT_STORAGE_ORDER, 1)
        U.upload(A)
        U.set_visibility(volumes=volumes, mask=hide)
        s = A
        _same_as_fresh(pkg, U, s, f"volumes and a mask (sh {sh})", sh, (volumes, hide))
        gone = rng.random(N) < 0.3
        assert U.remove(gone) == int((~gone).sum())
        s, hide = s.subset(~gone), hide[~gone]
        _same_as_fresh(pkg, U, s, f"30 % removed under it (sh {sh})", sh, (volumes, hide))
        s, hide = s.concat(B), np.concatenate([hide, np.zeros(B.n, bool)])
        assert s.n > N and U.add(B) == s.n
        assert U.get_add()["grows"] == 1 and U.get_add()["capacity"] == E.add_capacity(N, s.n)
        _same_as_fresh(pkg, U, s, f"200 added past the capacity (sh {sh})", sh, (volumes, hide))
        first, cnt = 100, 60
        vis = visible(s, hide)
        assert (~vis[first:first + cnt]).any() and vis[first:first + cnt].any(), "the range is not partly hidden: the case tests nothing"
        s = M._copy(pkg, s)
        s.alpha[first:first + cnt] = Cc.alpha[first:first + cnt]
        assert U.update_attrs(first, alpha=s.alpha[first:first + cnt]) == cnt
        _same_as_fresh(pkg, U, s, f"alphas of a partly hidden range (sh {sh})", sh, (volumes, hide))
        assert (~vis[-B.n:]).any() and (~vis[:-B.n]).any() and vis.any()
        assert U.remove(hidden=True) == int(vis.sum())
        s, hide = s.subset(vis), hide[vis]
        assert not hide.any() and U.get_visibility()[0].mask_splats == s.n
        _same_as_fresh(pkg, U, s, f"what was hidden removed (sh {sh})", sh, (volumes, hide))
        U.set_visibility()
        _same_as_fresh(pkg, U, s, f"the visibility cleared: the true alphas (sh {sh})", sh)
        assert U.stats()["uploads"] == 1 and U.stats()["n_splats"] == s.n
        _same_last_frame(pkg, U, s, f"visibility across the swap chain (sh {sh})")
