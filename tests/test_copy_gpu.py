"""Copying selected resident splats on the GPU: gsr_read_masked, gsr_read_masked_device, gsr_duplicate.

Everything is BIT-EXACT, there is no tolerance anywhere.  A masked read is held to read() indexed by copy_map (and read() to the host
arrays that were uploaded); a duplicate to a fresh upload of concat(R, R[rows]): the resident planes, the storage order and every later
frame.  The cloud, the comparators and the frame modes are test_move_gpu's: 357 splats = five full clusters of 64 and one of 37, so the
last mask word has 27 bits behind n; frames of 96 x 64."""
import ctypes as C

import numpy as np
import pytest

import test_move_gpu as M
import test_read_gpu as R
from helpers import HipBuffers

N = M.N
W, H = M.W, M.H
GSR_E_INVALID = -1
GUARD, FILL = R.GUARD, R.FILL
KEPT = ("uploads", "moves", "upload_ms", "move_ms", "n_splats")


def _masks(pkg, n=N, seed=21):
    """label -> packed words (None: the NULL mask) over n splats"""
    E = pkg.engine
    rng = np.random.default_rng(seed)
    bits = lambda idx: np.isin(np.arange(n), idx)
    out = {"empty": np.zeros(n, bool), "all": np.ones(n, bool), "first": bits([0]), "last": bits([n - 1]),
           "one cluster": bits(np.arange(64, 128)), "every other": np.arange(n) % 2 == 1, "random tenth": rng.random(n) < 0.1}
    out = {k: E.removal_mask(v) for k, v in out.items()}
    out["all and behind n"] = np.full((n + 31) // 32, 0xffffffff, np.uint32)
    out["NULL"] = None
    return out


def _rows(pkg, words, n):
    return np.arange(n, dtype=np.int32) if words is None else pkg.engine.copy_map(words, n)[0]


def _sel(pkg, words, n):
    return np.ones(n, bool) if words is None else pkg.engine.unpack_mask(words, n)


def _read_masked_guarded(pkg, eng, words, max_rows, names, mask_ptr=None):
    """gsr_read_masked through the C ABI into host destinations of max_rows rows between guard bytes -> (rc, m, {name: the rows})"""
    E, L = pkg.engine, pkg.load_library()
    r, raw, out = E.gsr_read_arrays(), {}, {}
    for k in names:
        dtype, width = R.ROW[k]
        raw[k] = np.full(GUARD + max_rows * width * np.dtype(dtype).itemsize + GUARD, FILL, np.uint8)
        setattr(r, k, raw[k].ctypes.data + GUARD)
    m = C.c_int64(-9)
    if mask_ptr is not None:
        rc = L.gsr_read_masked(eng.h, C.c_void_p(mask_ptr), 1, max_rows, C.byref(r), C.byref(m))
    else:
        rc = L.gsr_read_masked(eng.h, None if words is None else words.ctypes.data, 0, max_rows, C.byref(r), C.byref(m))
    for k in names:
        dtype, width = R.ROW[k]
        assert (raw[k][:GUARD] == FILL).all() and (raw[k][len(raw[k]) - GUARD:] == FILL).all(), f"{k}: a guard byte changed"
        out[k] = raw[k][GUARD:len(raw[k]) - GUARD].view(dtype).reshape((max_rows, width) if width > 1 else (max_rows,)).copy()
    return rc, m.value, out


def _assert_host_rows(pkg, out, m, want, names, label):
    """rows [0, m) of the guarded destinations are want's, the rows behind them still hold the fill pattern"""
    got = pkg.scenes.Splats(*[None if k not in out else out[k][:m] for k in R.NAMES])
    R._assert_rows(got, want, 0, m, names, label)
    for k in names:
        assert (out[k][m:].view(np.uint8) == FILL).all(), f"{label}: {k} was written behind row {m}"


def _read_masked_device_guarded(eng, hb, mask, max_rows, names, vpp=None, mask_is_device=True):
    """read_masked_device into device buffers of max_rows rows with guard bytes on either side -> (m, {name: float32 (max_rows, width)})"""
    width = {k: (3 * vpp if k == "sh" else R.DEV_WIDTH[k]) for k in names}
    base = {k: hb.upload(np.full(GUARD + max_rows * width[k] * 4 + GUARD, FILL, np.uint8)) for k in names}
    m = eng.read_masked_device({k: base[k] + GUARD for k in names}, mask, max_rows, sh_vec3_per_point=vpp if "sh" in names else None,
                               mask_is_device=mask_is_device)
    out = {}
    for k in names:
        raw = hb.download(base[k], (GUARD + max_rows * width[k] * 4 + GUARD,), np.uint8)
        assert (raw[:GUARD] == FILL).all() and (raw[len(raw) - GUARD:] == FILL).all(), f"{k}: a guard byte changed"
        out[k] = raw[GUARD:len(raw) - GUARD].view(np.float32).reshape(max_rows, width[k]).copy()
    return m, out


def _assert_device_rows(got, m, want_cloud, sh, vpp, names, label):
    if m:
        want = R._device_want(want_cloud, 0, m, sh and "sh" in names, vpp or 16)
        R._assert_device({k: got[k][:m] for k in names}, {k: want[k] for k in names}, label)
    for k in names:
        assert (got[k][m:].view(np.uint8) == FILL).all(), f"{label}: {k} was written behind row {m}"


def _stats_kept(st):
    return {k: st[k] for k in KEPT}


# ---- 1. masked read, both forms ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
@pytest.mark.parametrize("sh", (True, False))
def test_masked_read_both_forms(pkg, sh, order):
    E = pkg.engine
    A = M._cloud(pkg, 11, sh=sh)
    names = R._names(sh)
    dev_names = ("P", "alpha", "Cd", "scale", "orient") + (("sh",) if sh else ())
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.set_option(E.OPT_STORAGE_ORDER, order)
            U.upload(A)
            full = U.read()
            R._assert_rows(full, A, 0, N, names, "read")
            reads = U.get_read()["reads"]
            for label, words in _masks(pkg).items():
                rows = _rows(pkg, words, N)
                m = len(rows)
                assert m == int(_sel(pkg, words, N).sum())
                want = full.subset(rows)
                # the Python wrapper (a count call sizes the arrays), and the C ABI into destinations with room to spare
                got = U.read_masked(words)
                R._assert_rows(got, want, 0, m, names, f"{label}: read_masked")
                rc, cnt, out = _read_masked_guarded(pkg, U, words, m + 3, names)
                assert rc == 0 and cnt == m, label
                _assert_host_rows(pkg, out, m, want, names, f"{label}: gsr_read_masked")
                # the device form, from a device mask
                dmask = None if words is None else hb.upload(words)
                cnt, dout = _read_masked_device_guarded(U, hb, dmask, m + 3, dev_names, vpp=16 if sh else None)
                assert cnt == m, label
                _assert_device_rows(dout, m, want, sh, 16, dev_names, f"{label}: gsr_read_masked_device")
                reads += (3 if m else 0)
                info = U.get_read()
                assert info["reads"] == reads and (m == 0 or info["rows_last"] == m), (label, info)
            # each array alone (a P-only read is the cheap path), the three SH rows together
            words = _masks(pkg)["random tenth"]
            rows = _rows(pkg, words, N)
            want = full.subset(rows)
            for alone in [(k,) for k in names if k not in M.SH3] + ([M.SH3] if sh else []):
                R._assert_rows(U.read_masked(words, names=alone), want, 0, len(rows), alone, f"{alone} alone")
            dmask = hb.upload(words)
            for k in dev_names:
                vpps = (1, 15, 16) if k == "sh" else (None,)
                for vpp in vpps:
                    cnt, dout = _read_masked_device_guarded(U, hb, dmask, len(rows), (k,), vpp=vpp)
                    _assert_device_rows(dout, cnt, want, sh, vpp, (k,), f"device form, {k} alone, vpp {vpp}")
            # a host mask for the device form
            cnt, dout = _read_masked_device_guarded(U, hb, words, len(rows), ("P",), mask_is_device=False)
            _assert_device_rows(dout, cnt, want, sh, None, ("P",), "device form, host mask")
    finally:
        hb.free()


@pytest.mark.gpu
def test_masked_read_under_a_visibility(pkg):
    E = pkg.engine
    A = M._cloud(pkg, 11)
    volumes = [E.crop_box((0, 0, 0), 0.7)]
    hide = np.arange(N) % 3 == 0
    vis = E.visibility_eval(E.visibility_struct(volumes, hide)[0], A.P).astype(bool)
    words = _masks(pkg)["every other"]
    sel = _sel(pkg, words, N)
    assert (~vis & sel & (A.alpha != 0)).sum() > 10 and (vis & sel).sum() > 10, "the selection holds no hidden splat: the case tests nothing"
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.upload(A)
            U.set_visibility(volumes=volumes, mask=hide)
            geoA = U.debug_resident(E.RESIDENT_GEOA)
            want = A.subset(sel)
            R._assert_rows(U.read_masked(words), want, 0, want.n, R.NAMES, "under a visibility")          # the TRUE alpha of every row
            cnt, dout = _read_masked_device_guarded(U, hb, hb.upload(words), want.n, ("alpha", "P"))
            _assert_device_rows(dout, cnt, want, True, None, ("alpha", "P"), "under a visibility, device form")
            assert np.array_equal(U.debug_resident(E.RESIDENT_GEOA), geoA), "the read changed geoA"
            assert U.get_visibility()[1] == int((~vis).sum())
    finally:
        hb.free()


# ---- 2. several blocks ---------------------------------------------------------------------------------------------------------
def _blocks_case(pkg):
    E = pkg.engine
    block = E.COPY_BLOCK
    n = 2 * block + 64 + 5
    s = M._cloud(pkg, 31, n=n)
    sel = np.random.default_rng(5).random(n) < 0.1
    sel[[block - 1, block, 2 * block]] = True
    return s, sel, block


@pytest.mark.gpu
def test_masked_read_over_several_blocks(pkg):
    s, sel, block = _blocks_case(pkg)
    n = s.n
    assert n % block and n % 32 and sel[2 * block:].sum() > 1
    words = pkg.engine.removal_mask(sel)
    words[-1] |= np.uint32((0xffffffff << (n % 32)) & 0xffffffff)            # garbage behind n
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.upload(s)
            want = s.subset(sel)
            R._assert_rows(U.read_masked(words), want, 0, want.n, R.NAMES, "three blocks")
            cnt, dout = _read_masked_device_guarded(U, hb, hb.upload(words), want.n + 1, ("P", "alpha", "sh"), vpp=16)
            assert cnt == want.n
            _assert_device_rows(dout, cnt, want, True, 16, ("P", "alpha", "sh"), "three blocks, device form")
    finally:
        hb.free()


@pytest.mark.gpu
def test_duplicate_over_several_blocks(pkg):
    s, sel, block = _blocks_case(pkg)
    with pkg.Engine(0) as U:
        U.upload(s)
        m, total = U.duplicate(sel)
        assert (m, total) == (int(sel.sum()), s.n + int(sel.sum()))
        got = M._planes(U)
    M._assert_same_planes(got, M._fresh_planes(pkg, s.concat(s.subset(sel))), "a duplicate over three blocks")


# ---- 2b. a selection whose rows do not fit the staging arena the upload left ------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", (N, 100003))
def test_a_selection_that_outgrows_the_staging_arena(pkg, n):
    """A cloud without SH stages 36 bytes per splat at its upload; a masked read of nearly all of it by a host mask needs the mask, the
    bitmap, the row list AND 36 bytes per row, a duplicate 4 + 32 bytes per splat of the larger cloud: both must replace the arena
    between the count and the compaction, and what the count left in the old one is gone.  The arena's capacity before and after
    says that the case still does that; the results are held bit for bit."""
    s = M._cloud(pkg, 41, sh=False, n=n)
    sel = np.arange(n) % 997 != 5
    names = R._names(False)
    want_rows = s.subset(sel)
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.upload(s)
            cap0 = U.debug_stage_bytes()
            assert 0 < cap0 < 40 * n + 4096
            R._assert_rows(U.read_masked(sel), want_rows, 0, want_rows.n, names, "a masked read that replaces the arena")
            cap1 = U.debug_stage_bytes()
            assert cap1 > cap0, "the masked read fitted the arena of the upload: the case tests nothing"
            R._assert_rows(U.read_masked(sel), want_rows, 0, want_rows.n, names, "the same read again, the arena large enough")
            assert U.debug_stage_bytes() == cap1
            # the device form stages the row list only: it fits, and agrees
            cnt, dout = _read_masked_device_guarded(U, hb, pkg.engine.removal_mask(sel), want_rows.n, ("P", "alpha", "Cd"), mask_is_device=False)
            _assert_device_rows(dout, cnt, want_rows, False, None, ("P", "alpha", "Cd"), "device form beside it")
        with pkg.Engine(0) as U:
            U.upload(s)
            cap0 = U.debug_stage_bytes()
            assert U.duplicate(sel) == (want_rows.n, n + want_rows.n)
            assert U.debug_stage_bytes() > cap0, "the duplicate fitted the arena of the upload: the case tests nothing"
            got = M._planes(U, sh=False)
            R._assert_rows(U.read(), s.concat(want_rows), 0, n + want_rows.n, names, "read after a duplicate that replaces the arena")
        M._assert_same_planes(got, M._fresh_planes(pkg, s.concat(want_rows), sh=False), "a duplicate that replaces the arena")
    finally:
        hb.free()


# ---- 3. max_rows ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_max_rows(pkg):
    E, L = pkg.engine, pkg.load_library()
    A = M._cloud(pkg, 11)
    cam = M._cams(pkg, [2])[0]
    words = _masks(pkg)["random tenth"]
    m = int(_sel(pkg, words, N).sum())
    assert m > 2
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.upload(A)
            frame = U.render(cam).copy()
            planes, st, reads = M._planes(U), _stats_kept(U.stats()), U.get_read()["reads"]
            rc, cnt, out = _read_masked_guarded(pkg, U, words, m - 1, R.NAMES)
            assert rc == GSR_E_INVALID and cnt == m and b"gsr_read_masked" in L.gsr_last_error()
            for k in R.NAMES:
                assert (out[k].view(np.uint8) == FILL).all(), f"{k} was written by a refused read"
            with pytest.raises(E.GsrError):
                _read_masked_device_guarded(U, hb, hb.upload(words), m - 1, ("P", "alpha", "sh"), vpp=16)
            base = hb.upload(np.full((m - 1) * 12, FILL, np.uint8))
            d, cnt = E.gsr_device_out(), C.c_int64(-1)
            d.P = base
            assert L.gsr_read_masked_device(U.h, words.ctypes.data, 0, m - 1, C.byref(d), C.byref(cnt)) == GSR_E_INVALID and cnt.value == m
            assert (hb.download(base, ((m - 1) * 12,), np.uint8) == FILL).all(), "P was written by a refused read"
            # the count form: every destination NULL (or no struct at all); max_rows is not looked at
            for out_struct in (None, C.byref(E.gsr_read_arrays())):
                cnt = C.c_int64(-1)
                assert L.gsr_read_masked(U.h, words.ctypes.data, 0, 0, out_struct, C.byref(cnt)) == 0 and cnt.value == m
            cnt = C.c_int64(-1)
            assert L.gsr_read_masked_device(U.h, words.ctypes.data, 0, -5, None, C.byref(cnt)) == 0 and cnt.value == m
            assert U.read_masked_device({}, words, mask_is_device=False) == m
            # exactly max_rows fits
            rc, cnt, out = _read_masked_guarded(pkg, U, words, m, ("P",))
            assert rc == 0 and cnt == m
            assert U.get_read()["reads"] == reads + 1, "a refusal or a count was counted as a read"
            M._assert_same_planes(M._planes(U), planes, "refused reads")
            assert _stats_kept(U.stats()) == st
            assert np.array_equal(U.render(cam), frame)
    finally:
        hb.free()


# ---- 4. a read changes nothing -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_masked_read_changes_nothing(pkg):
    E = pkg.engine
    A = M._cloud(pkg, 11)
    cam = M._cams(pkg, [2])[0]
    words = _masks(pkg)["every other"]
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.upload(A)
            frame = U.render(cam).copy()
            assert (frame[..., 3] > 0).sum() > 100
            U.render(cam)
            st = U.stats()
            assert st["sorts_skipped"] >= 1
            planes = M._planes(U)
            want = A.subset(_sel(pkg, words, N))
            R._assert_rows(U.read_masked(words), want, 0, want.n, R.NAMES, "between two frames")
            ptrs = {"P": hb.alloc(N * 12), "sh": hb.alloc(N * 180)}
            assert U.read_masked_device(ptrs, hb.upload(words), N, sh_vec3_per_point=15) == want.n
            again = U.render(cam)
            st2 = U.stats()
            assert st2["sorts_skipped"] == st["sorts_skipped"] + 1, "the read invalidated the cached depth order"
            assert np.array_equal(again.view(np.uint32), frame.view(np.uint32))
            assert _stats_kept(st2) == _stats_kept(st)
            assert U.get_duplicate()["duplicates"] == 0 and U.get_add()["grows"] == 0
            M._assert_same_planes(M._planes(U), planes, "a masked read between frames")

        # a culled regime: the frames around a masked read are those of a context that never reads
        cams = M._cams(pkg, range(6))

        def run(read):
            with pkg.Engine(0) as V:
                V.set_option(E.OPT_OCCLUSION_CULL, 2)
                V.upload(A)
                out = []
                for k, c in enumerate(cams):
                    if read and k == 3:
                        V.read_masked(words, names=("P", "alpha", "Cd"))
                    out.append(V.render(c).copy())
                s = V.stats()
                return out, (s["frames_culled"], s["frames_repaired"], s["sorts_skipped"])

        want_frames, want_st = run(False)
        got_frames, got_st = run(True)
        assert got_st == want_st
        for k in range(len(cams)):
            assert np.array_equal(got_frames[k], want_frames[k]), k
    finally:
        hb.free()


# ---- 5. duplicate, resident bits -----------------------------------------------------------------------------------------------
def _kinds(order, n_old):
    """per cluster of the storage order: 'old', 'new' or 'mixed'"""
    out = []
    for at in range(0, len(order), 64):
        new = order[at:at + 64] >= n_old
        out.append("new" if new.all() else "mixed" if new.any() else "old")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("order", (1, 0))
@pytest.mark.parametrize("sh", (True, False))
def test_duplicate_resident_bits(pkg, sh, order):
    E = pkg.engine
    A = M._cloud(pkg, 11, sh=sh)
    names = R._names(sh)
    mixed, grew, fitted = 0, 0, 0
    for label, words in _masks(pkg).items():
        for room in (False, True):
            with pkg.Engine(0) as U:
                U.set_option(E.OPT_STORAGE_ORDER, order)
                U.upload(A)
                base = A
                if room:                                                # a removal makes room: the duplicate fits the capacity
                    gone = np.arange(N) >= 157
                    assert U.remove(gone) == 157
                    base = A.subset(~gone)
                n0 = base.n
                w = None if words is None else words[:(n0 + 31) // 32].copy()
                rows = _rows(pkg, w, n0)
                m = len(rows)
                if room and m > 157:
                    continue                                            # (does not fit the room made: the growing cases cover it)
                before, st0 = U.get_add(), U.stats()
                R._assert_rows(U.read(), base, 0, n0, names, f"{label}: before")
                got_m, total = U.duplicate(w)
                assert (got_m, total) == (m, n0 + m), label
                want_cloud = base.concat(base.subset(rows))
                got = M._planes(U, sh)
                after, st1, dup = U.get_add(), U.stats(), U.get_duplicate()
                cap = E.add_capacity(before["capacity"], n0 + m)
                assert after["capacity"] == cap and after["grows"] == before["grows"] + (cap != before["capacity"]), (label, before, after)
                assert after["adds"] == before["adds"] and after["added_last"] == before["added_last"]
                assert st1["n_splats"] == n0 + m and st1["uploads"] == st0["uploads"] and st1["moves"] == st0["moves"]
                assert dup["duplicates"] == (1 if m else 0) and dup["copied_last"] == m
                R._assert_rows(U.read(), want_cloud, 0, n0 + m, names, f"{label}: read after the duplicate")
            if m == 0:
                continue
            grew += cap != before["capacity"]
            fitted += cap == before["capacity"]
            with pkg.Engine(0) as F:
                F.set_option(E.OPT_STORAGE_ORDER, order)
                F.upload(want_cloud)
                want = M._planes(F, sh)
                order_f = F.debug_storage_order(want_cloud.n)
            M._assert_same_planes(got, want, f"{label}, room {room}")
            kinds = _kinds(order_f, n0)
            mixed += "mixed" in kinds
    assert grew >= 3 and fitted >= 3, f"the cases no longer cover a duplicate that grows ({grew}) and one that fits ({fitted})"
    if order == 1:
        assert mixed >= 1, "no case has clusters that mix originals and copies: the cases test nothing of the re-order"


# ---- 6. duplicate equals masked read plus add ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("room", (False, True))
def test_duplicate_equals_masked_read_plus_add(pkg, room):
    E = pkg.engine
    A = M._cloud(pkg, 11)
    cam = M._cams(pkg, [3])[0]
    volumes = [E.crop_box((0, 0, 0), 0.7)]
    hide = np.arange(N) % 3 == 0
    gone = np.arange(N) % 5 == 4
    n0 = N - int(gone.sum()) if room else N
    sel = np.random.default_rng(8).random(n0) < 0.15
    assert not room or int(sel.sum()) <= int(gone.sum())
    results = []
    for way in ("duplicate", "read_masked + add"):
        with pkg.Engine(0) as U:
            U.upload(A)
            U.set_visibility(volumes=volumes, mask=hide)
            if room:
                assert U.remove(gone) == n0
            cap0 = U.get_add()["capacity"]
            hidden0 = U.get_visibility()[1]
            assert hidden0 > 10
            if way == "duplicate":
                m, total = U.duplicate(sel)
            else:
                rows = U.read_masked(sel)
                m, total = rows.n, U.add(rows)
            assert (m, total) == (int(sel.sum()), n0 + int(sel.sum()))
            assert (U.get_add()["capacity"] == cap0) == room, "the case no longer grows / fits as its name says"
            vis, hidden = U.get_visibility()
            results.append({"planes": M._planes(U), "hidden": hidden, "n_volumes": vis.n_volumes, "mask_splats": vis.mask_splats,
                            "read": U.read(), "frame": U.render(cam).copy(), "grows": U.get_add()["grows"]})
            assert hidden > hidden0, "no copy is hidden by the volumes: the case tests nothing of the visibility"
    a, b = results
    M._assert_same_planes(a["planes"], b["planes"], "duplicate vs read_masked + add")
    assert (a["hidden"], a["n_volumes"], a["mask_splats"], a["grows"]) == (b["hidden"], b["n_volumes"], b["mask_splats"], b["grows"])
    R._assert_rows(a["read"], b["read"], 0, b["read"].n, R.NAMES, "the true alphas and every other row")
    assert (a["frame"][..., 3] > 0).sum() > 100 and np.array_equal(a["frame"], b["frame"])


# ---- 7. duplicate, range_mask, transform, frames -------------------------------------------------------------------------------
def _dup_and_transform(pkg, U, A, sel):
    """duplicate the selection and move the copies aside -> the edited cloud on the host"""
    E = pkg.engine
    x = E.xform(axis_angle=((0.3, 1.0, 0.2), 40.0), scale=0.8, translate=(0.25, -0.1, 0.15))
    m, total = int(sel.sum()), A.n + int(sel.sum())
    copies = E.range_mask(A.n, m, total)
    if U is not None:
        assert U.duplicate(sel) == (m, total)
        assert U.transform(x, copies) == m
    return E.transform_eval(x, A.concat(A.subset(sel)), copies)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["cull 0", "cull 2", "cull 3", "lazy 0", "lazy 2", "sort cache 2", "depth-tested", "rgba16f",
                                  "shard 1/2 interleaved", "shard 1/2 bands"])
def test_frames_after_a_duplicate_and_a_transform(pkg, mode):
    A = M._cloud(pkg, 11)
    sel = np.random.default_rng(9).random(N) < 0.3
    opts, render, prepare = M._frame_modes(pkg)[mode]
    draw = render or (lambda eng, c: eng.render(c))
    cams = M._cams(pkg, range(8))
    with pkg.Engine(0) as U:
        for k, v in opts:
            U.set_option(k, v)
        if prepare:
            prepare(U)
        U.upload(A)
        for c in cams[:5]:
            draw(U, c)
        edited = _dup_and_transform(pkg, U, A, sel)
        got = [draw(U, c).copy() for c in cams[5:]]
    want = M._fresh_frames(pkg, edited, cams[5:], opts, render=render, prepare=prepare)
    stale = M._fresh_frames(pkg, A, cams[5:], opts, render=render, prepare=prepare)
    for k in range(len(want)):
        assert not np.array_equal(want[k], stale[k]), f"{mode}: the copies do not show in frame {k}: the case tests nothing"
        assert np.array_equal(got[k], want[k]), (f"{mode}: frame {k} after the duplicate differs from a fresh upload's in "
                                                 f"{int((got[k] != want[k]).any(axis=2).sum())} pixels")


@pytest.mark.gpu
def test_frames_after_a_duplicate_two_in_flight_device_target(pkg):
    E = pkg.engine
    A = M._cloud(pkg, 11)
    sel = np.random.default_rng(9).random(N) < 0.3
    cams = M._cams(pkg, range(8))
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.set_option(E.OPT_FRAMES_IN_FLIGHT, 2)
            U.set_option(E.OPT_DEFERRED_CHECK, 1)
            U.upload(A)
            outs = [hb.alloc(W * H * 16) for _ in cams]
            for c, o in zip(cams[:5], outs[:5]):
                U.render_to_device(c, o)
            edited = _dup_and_transform(pkg, U, A, sel)                  # (no synchronisation by the caller)
            for c, o in zip(cams[5:], outs[5:]):
                U.render_to_device(c, o)
            U.synchronize()
            got = [hb.download(o, (H, W, 4)) for o in outs]
        before = M._fresh_frames(pkg, A, cams[:5])
        for k in range(5):
            assert np.array_equal(got[k], before[k]), f"frame {k}, queued before the duplicate, was disturbed by it"
        want = M._fresh_frames(pkg, edited, cams[5:])
        for k in range(len(want)):
            assert np.array_equal(got[5 + k], want[k]), f"frame {k} after the duplicate"
    finally:
        hb.free()


# ---- 8. nothing selected -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_an_empty_selection_changes_nothing(pkg):
    A = M._cloud(pkg, 11)
    cam = M._cams(pkg, [2])[0]
    garbage = np.zeros((N + 31) // 32, np.uint32)
    garbage[-1] = np.uint32((0xffffffff << (N % 32)) & 0xffffffff)
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.upload(A)
            frame = U.render(cam).copy()
            U.render(cam)
            st, planes, add0 = U.stats(), M._planes(U), U.get_add()
            for k, words in enumerate((np.zeros(N, bool), garbage)):
                assert U.duplicate(words) == (0, N)
                assert U.duplicate_device(hb.upload(garbage)) == (0, N)
                assert np.array_equal(U.render(cam), frame)
            st2 = U.stats()
            assert st2["sorts_skipped"] == st["sorts_skipped"] + 2, "an empty duplicate invalidated the cached depth order"
            assert _stats_kept(st2) == _stats_kept(st)
            assert U.get_duplicate()["duplicates"] == 0 and U.get_add() == add0
            M._assert_same_planes(M._planes(U), planes, "an empty duplicate")
    finally:
        hb.free()


# ---- 9. device mask ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_mask(pkg):
    E, L = pkg.engine, pkg.load_library()
    A = M._cloud(pkg, 11)
    cam = pkg.camera.make_camera(W, H, sh_order=3, frame=1)
    region = E.select_region(rect=(10, 8, 70, 50))
    hb = HipBuffers()
    try:
        size = 2 << 20                                                  # (a multiple of any granularity the allocator may round to)
        room = hb.alloc(size)
        n_words = (N + 31) // 32
        dev = hb.upload(np.zeros(n_words, np.uint32))
        pageable = np.zeros(n_words, np.uint32)
        with pkg.Engine(0) as U:
            U.upload(A)
            hit, nset = U.select_device(cam, region, dev)
            assert 10 < nset < N - 10, "the region selects nothing or everything: the case tests nothing"
            sel = E.unpack_mask(hb.download(dev, (n_words,), np.uint32), N)
            assert int(sel.sum()) == nset
            planes = M._planes(U)
            m, total = C.c_int64(-1), C.c_int64(-1)
            # refused by the pointer check, before anything is launched (the pure query first: no verb is handed a pointer it would take)
            short = room + size - (n_words - 1) * 4                     # one word short of the end of its allocation
            d = E.gsr_device_out()
            d.P = hb.alloc(N * 12)
            for label, ptr, nbytes in (("pageable", pageable.ctypes.data, pageable.nbytes), ("one word short", short, n_words * 4)):
                assert not U.check_device_source(ptr, nbytes), label
                assert L.gsr_duplicate(U.h, C.c_void_p(ptr), 1, C.byref(m), C.byref(total)) == GSR_E_INVALID, label
                assert b"gsr_duplicate" in L.gsr_last_error(), label
                assert L.gsr_read_masked(U.h, C.c_void_p(ptr), 1, 0, None, C.byref(m)) == GSR_E_INVALID, label
                assert L.gsr_read_masked_device(U.h, C.c_void_p(ptr), 1, N, C.byref(d), C.byref(m)) == GSR_E_INVALID, label
                M._assert_same_planes(M._planes(U), planes, label)
            # a destination too small for max_rows, whatever the selection holds
            small = E.gsr_device_out()
            small.P = room + size - (nset + 1) * 12 + 4                 # four bytes short of nset + 1 rows
            assert not U.check_device_source(small.P, (nset + 1) * 12) and U.check_device_source(small.P, nset * 12)
            assert L.gsr_read_masked_device(U.h, C.c_void_p(dev), 1, nset + 1, C.byref(small), C.byref(m)) == GSR_E_INVALID
            assert b"gsr_read_masked_device" in L.gsr_last_error()
            assert (m.value, total.value) == (-1, -1)
            assert U.get_duplicate()["duplicates"] == 0 and U.stats()["n_splats"] == N and U.get_read()["reads"] == 0
            # the mask straight from select_device
            want_rows = A.subset(sel)
            R._assert_rows(pkg.scenes.Splats(*[_read_masked_guarded(pkg, U, None, nset, R.NAMES, mask_ptr=dev)[2].get(k) for k in R.NAMES]),
                           want_rows, 0, nset, R.NAMES, "gsr_read_masked from a device mask")
            assert U.duplicate_device(dev) == (nset, N + nset)
            assert U.get_duplicate()["ms"][0] == 0.0                    # nothing crossed the link
            got = M._planes(U)
        with pkg.Engine(0) as V:
            V.upload(A)
            assert V.duplicate(sel) == (nset, N + nset)
            M._assert_same_planes(got, M._planes(V), "device mask vs host mask")
        M._assert_same_planes(got, M._fresh_planes(pkg, A.concat(want_rows)), "device mask")
    finally:
        hb.free()


# ---- 10. an edit chain ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_edit_chain(pkg):
    """select, duplicate, transform the copies, grade them, remove the originals, read: against the same chain on host arrays"""
    E = pkg.engine
    A = M._cloud(pkg, 11)
    cam = pkg.camera.make_camera(W, H, sh_order=3, frame=1)
    x = E.xform(axis_angle=((0.0, 1.0, 0.0), 90.0), translate=(0.4, 0.0, 0.0))
    rule = E.grade_rule(np.asarray([[0.2, 0.7, 0.1], [0.1, 0.8, 0.1], [0.3, 0.3, 0.4]], np.float32), b=(0.02, 0.0, -0.01), alpha_gain=0.75)
    with pkg.Engine(0) as U:
        U.upload(A)
        sel, hit, nset = U.select(cam, E.select_region(rect=(10, 8, 70, 50)))
        assert 10 < nset < N - 10
        m, total = U.duplicate(sel)
        assert (m, total) == (nset, N + nset)
        copies = E.unpack_mask(E.range_mask(N, m, total), total)
        assert U.transform(x, copies) == m
        assert U.grade(rule, copies) == m
        originals = np.concatenate([sel, np.zeros(m, bool)])
        assert U.remove(originals) == N
        got = U.read()
        got_planes = M._planes(U)
    want = A.concat(A.subset(E.copy_map(sel)[0]))
    want = E.grade_eval(rule, E.transform_eval(x, want, copies), copies)
    new_index, left = E.remove_map(originals)
    assert left == N
    want = want.subset(new_index >= 0)
    R._assert_rows(got, want, 0, N, R.NAMES, "the chain")
    M._assert_same_planes(got_planes, M._fresh_planes(pkg, want), "the chain")


# ---- 11. refusals leave the context alone --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_leave_the_context_alone(pkg):
    E, L = pkg.engine, pkg.load_library()
    A = M._cloud(pkg, 11)
    cam = M._cams(pkg, [2])[0]
    words = _masks(pkg)["random tenth"]
    m, total = C.c_int64(-7), C.c_int64(-7)
    shrow = np.zeros((N, 16), np.uint16)
    p = words.ctypes.data

    def sh_wanted(n_arrays):
        r = E.gsr_read_arrays()
        for k in M.SH3[:n_arrays]:
            setattr(r, k, shrow.ctypes.data)
        return r

    def verbs(eng, r=None):
        r = r if r is not None else sh_wanted(3)
        return {"gsr_duplicate": lambda: L.gsr_duplicate(eng.h, p, 0, C.byref(m), C.byref(total)),
                "gsr_read_masked": lambda: L.gsr_read_masked(eng.h, p, 0, N, C.byref(r), C.byref(m)),
                "gsr_read_masked_device": lambda: L.gsr_read_masked_device(eng.h, p, 0, 0, None, C.byref(m))}

    with pkg.Engine(0) as U:
        for name, fn in verbs(U).items():                               # before any upload
            assert fn() == GSR_E_INVALID and b"no geometry" in L.gsr_last_error() and name.encode() in L.gsr_last_error(), name
        U.upload(A)
        planes, frame = M._planes(U), U.render(cam).copy()
        d = E.gsr_device_out()
        d.reserved_ = 1
        cases = {
            "one SH array": lambda: L.gsr_read_masked(U.h, p, 0, N, C.byref(sh_wanted(1)), C.byref(m)),
            "two SH arrays": lambda: L.gsr_read_masked(U.h, p, 0, N, C.byref(sh_wanted(2)), C.byref(m)),
            "max_rows < 0": lambda: L.gsr_read_masked(U.h, p, 0, -1, C.byref(sh_wanted(3)), C.byref(m)),
            "reserved_": lambda: L.gsr_read_masked_device(U.h, p, 0, N, C.byref(d), C.byref(m)),
        }
        for label, fn in cases.items():
            assert fn() == GSR_E_INVALID, label
            M._assert_same_planes(M._planes(U), planes, label)
            assert np.array_equal(U.render(cam), frame), label
        assert (m.value, total.value) == (-7, -7) and not shrow.any()
        # an upload in progress (gsr_upload_begin itself gave the resident cloud up: what can be held is the refusal and its text)
        assert L.gsr_upload_begin(U.h, N, 1, None) == 0
        for name, fn in verbs(U).items():
            assert fn() == GSR_E_INVALID and b"upload in progress" in L.gsr_last_error(), name
        assert L.gsr_upload_abort(U.h) == 0
        U.upload(A)
        M._assert_same_planes(M._planes(U), planes, "uploaded again after the refusals")
        assert U.duplicate(words)[1] == N + int(_sel(pkg, words, N).sum())
    with pkg.Engine(0) as V:                                            # SH arrays wanted for a cloud uploaded without SH
        V.upload(M._cloud(pkg, 11, sh=False))
        planes, frame = M._planes(V, sh=False), V.render(cam).copy()
        assert verbs(V)["gsr_read_masked"]() == GSR_E_INVALID and b"without SH" in L.gsr_last_error()
        d = E.gsr_device_out()
        d.sh, d.sh_vec3_per_point = 4096, 16                            # (refused before the pointer is looked at)
        assert L.gsr_read_masked_device(V.h, p, 0, N, C.byref(d), C.byref(m)) == GSR_E_INVALID and b"without SH" in L.gsr_last_error()
        M._assert_same_planes(M._planes(V, sh=False), planes, "SH wanted without SH")
        assert np.array_equal(V.render(cam), frame) and not shrow.any() and m.value == -7


# ---- 12. several ranks ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi_matches_single_context(pkg):
    E = pkg.engine
    A = M._cloud(pkg, 11)
    sel = np.random.default_rng(9).random(N) < 0.3
    cams = M._cams(pkg, range(4))
    m = int(sel.sum())
    edited = A.concat(A.subset(sel))
    with pkg.MultiEngine([0, 0], E.TRANSPORT_COPY) as X:
        X.upload(A)
        for c in cams[:2]:
            X.render(c)
        R._assert_rows(X.read_masked(sel), A.subset(sel), 0, m, R.NAMES, "MultiEngine.read_masked")
        R._assert_rows(X.read_masked(sel, names=("P",)), A.subset(sel), 0, m, ("P",), "MultiEngine.read_masked, P alone")
        assert X.duplicate(np.zeros(N, bool)) == (0, N)
        assert X.duplicate(sel) == (m, N + m)
        got = [X.render(c).copy() for c in cams[2:]]
        st = [X.stats(r) for r in range(2)]
        assert [s["n_splats"] for s in st] == [N + m] * 2 and [s["uploads"] for s in st] == [1, 1]
        R._assert_rows(X.read(), edited, 0, N + m, R.NAMES, "MultiEngine.read after the duplicate")
    want = M._fresh_frames(pkg, edited, cams[2:])
    for k in range(len(want)):
        assert np.array_equal(got[k], want[k]), f"frame {k} of two ranks after the duplicate"
