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


# ---- 4. one mask intake: a host mask and the same words in device memory ----------------------------------------------------------
def _intake_masks(pkg, n):
    """(label, packed words) of a fixed-seed selection over n splats -- the first and the last splat selected -- and of one with no bit
    set below n; in the last word of both every bit at and behind n is set, which no verb may read"""
    rng = np.random.default_rng(40 + n)
    sel = rng.random(n) < 0.4
    sel[0] = sel[-1] = True
    out = []
    for label, bits in (("selection", sel), ("no bit below n", np.zeros(n, bool))):
        words = pkg.engine.pack_mask(bits)
        if n % 32:
            words[-1] |= np.uint32((0xffffffff << (n % 32)) & 0xffffffff)
        out.append((label, words))
    return out


def _assert_same_splats(got, want, label):
    for k in ("P", "Cd", "alpha", "scale", "orient", "shx", "shy", "shz"):
        g, w = getattr(got, k), getattr(want, k)
        assert (g is None) == (w is None), (label, k)
        if w is not None:
            assert g.shape == w.shape and np.array_equal(g.view(np.uint8), w.view(np.uint8)), (label, k)


@pytest.mark.gpu
@pytest.mark.parametrize("n", (1, 33, 64, 4097))
def test_one_mask_intake_host_and_device(pkg, n):
    """remove, duplicate, transform, grade and read_masked take a mask through one intake: from host words and from the same words
    in device memory each verb, on a fresh upload, returns the host model's count, leaves bit for bit the model's cloud (read()), and
    advances its tally by one with *_last = that count.  n: a word edge (1, 33), a wave edge (64), one past GSR_REMOVE_BLOCK (4097).
    A mask with no bit below n selects nothing: every verb counts 0 and the cloud stays the upload (remove, duplicate and a masked read
    then leave their tallies as they were -- they count calls that did something --, transform and grade count the call)"""
    import ctypes as Ct
    from helpers import HipBuffers
    E, L = pkg.engine, pkg.load_library()
    A = M._cloud(pkg, 31, n=n)
    x = E.xform(axis_angle=((0.3, 1.0, 0.2), 40.0), scale=1.5, translate=(0.1, -0.2, 0.3), pivot=(0.05, 0.0, 0.0))
    rule = E.grade_prepare(E.grade_params(exposure=0.3, saturation=0.7, alpha_gain=0.8, alpha_offset=0.05))
    assert rule["flags"] == E.GRADE_COLOUR | E.GRADE_ALPHA

    def read_masked_device(U, dptr, words):
        verb = lambda ptr, max_rows, r, m: L.gsr_read_masked(U.h, Ct.c_void_p(dptr), 1, max_rows, r, m)    # noqa: E731
        return E._read_masked_splats(verb, (n, True), words, None)

    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            for label, words in _intake_masks(pkg, n):
                dptr = hb.upload(words)
                sel = E.unpack_mask(words, n)
                rows, m = E.copy_map(words, n)
                _, left = E.remove_map(words, n)
                assert m == int(sel.sum()) and left == n - m and (m > 0) == (label == "selection"), (label, m, left)
                # verb -> (run from host words, run from device words: the count; the tally's getter and keys; the model's cloud)
                verbs = {
                    "remove": (lambda: n - U.remove(words), lambda: n - U.remove_device(dptr), U.get_removal, "removals", "removed_last",
                               A.subset(~sel)),
                    "duplicate": (lambda: U.duplicate(words)[0], lambda: U.duplicate_device(dptr)[0], U.get_duplicate, "duplicates",
                                  "copied_last", A.concat(A.subset(rows))),
                    "transform": (lambda: U.transform(x, words), lambda: U.transform_device(x, dptr), U.get_transform, "transforms",
                                  "moved_last", E.transform_eval(x, A, words)),
                    "grade": (lambda: U.grade(rule, words), lambda: U.grade_device(rule, dptr), U.get_grade, "grades", "graded_last",
                              E.grade_eval(rule, A, words)),
                    "read_masked": (lambda: U.read_masked(words), lambda: read_masked_device(U, dptr, words),
                                    U.get_read, "reads", "rows_last", A),
                }
                for verb, (host, device, tally, calls, key, want) in verbs.items():
                    runs = []
                    for form, run in (("host", host), ("device", device)):
                        case = f"n {n}, {label}, {verb} from a {form} mask"
                        U.upload(A)
                        before = tally()
                        got = run()
                        after = tally()
                        advanced = 1 if (m or verb in ("transform", "grade")) else 0
                        assert after[calls] == before[calls] + advanced, (case, before, after)
                        if advanced:
                            assert after[key] == m, (case, after)
                        if verb == "read_masked":
                            _assert_same_splats(got, A.subset(rows), case)
                            got = got.P.shape[0]
                        assert got == m, (case, got, m)
                        cloud = U.read()
                        _assert_same_splats(cloud, want, case)
                        runs.append((got, cloud))
                    assert runs[0][0] == runs[1][0], (n, label, verb)
                    _assert_same_splats(runs[1][1], runs[0][1], f"n {n}, {label}, {verb}: device run against host run")
    finally:
        hb.free()
