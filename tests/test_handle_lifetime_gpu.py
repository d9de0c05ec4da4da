"""What a context allocates goes when it is destroyed (csrc/gsr_host_buffers.h: the owning handles, counted by gsr_debug_live_handles).

One engine drives every lazily allocated object of the host code once -- the staging buffers of host targets, depth buffers, planes
and backgrounds, the wire overlay, the row mailboxes, the second frame slot, a front slab, the band copies' stream and events, the
position-keyed order, the visibility's buffers, the spare planes, the capacity growth of an add, the inverse permutation, a second
upload -- then the counts must be back where they were.  The read at the end of the edit chain is held, bit for bit, to the host arrays
(test_read_gpu's helper), so the verbs really ran."""
import gc

import numpy as np
import pytest

import test_move_gpu as M
import test_read_gpu as R
from helpers import HipBuffers

N = 300                      # four full clusters of 64 and one of 44
W = H = 48


@pytest.mark.gpu
def test_a_context_releases_every_handle(pkg):
    E = pkg.engine
    A, B = M._cloud(pkg, 11, n=N), M._cloud(pkg, 12, n=N)
    new, small = M._cloud(pkg, 13, n=400), M._cloud(pkg, 14, n=100)
    cam, cam2 = (pkg.camera.make_camera(W, H, sh_order=3, frame=f) for f in (1, 2))
    tall = pkg.camera.make_camera(W, 256, sh_order=3, frame=1)      # 16 tile rows: a host target is copied back band by band
    depth = np.ones((H, W), np.float32)
    bg = np.full((H, W, 4), 0.25, np.float32)
    names = R._names(True)
    gc.collect()                                                    # (an engine another test dropped goes now, not in the middle)
    base = E.live_handles()
    hb = HipBuffers()
    try:
        with pkg.Engine(0) as U:
            U.upload(A)
            U.render(cam)
            U.render_to_device(cam, hb.alloc(W * H * 16))
            U.render_depth(cam, depth)
            U.render_aov(cam)
            U.render_over(cam, bg)
            U.render_wire(cam)
            U.render(tall)
            U.set_option(E.OPT_ROW_WORK, 1)
            U.render(cam)
            assert U.read_row_work(H)[0].shape == (H // 16,)
            U.set_option(E.OPT_FRAMES_IN_FLIGHT, 2)
            U.render(cam); U.render(cam2)
            U.set_option(E.OPT_FRAMES_IN_FLIGHT, 1)
            U.set_option(E.OPT_FRONT_SLAB, 2)
            U.render(cam2)
            U.set_option(E.OPT_FRONT_SLAB, 1)
            U.set_option(E.OPT_SORT_CACHE, 2)
            U.render(cam); U.render(cam)
            U.set_visibility(volumes=[E.crop_box((0, 0, 0), 0.7)], mask=np.arange(N) % 3 == 0)
            # the edit chain, under the visibility: s is what the context must hold
            s = M._copy(pkg, A)
            rows = {k: np.ascontiguousarray(getattr(B, k)[20:30]) for k in names if k != "P"}
            assert U.update_attrs(20, **rows) == 10
            for k, v in rows.items():
                getattr(s, k)[20:30] = v
            s = M._move(pkg, U, s, B.P[100:110], 100)
            gone = np.zeros(N, bool)
            gone[5:285:7] = True
            assert gone.sum() == 40 and U.remove(gone) == N - 40
            s = s.subset(~gone).concat(new)
            assert U.add(new) == s.n and U.get_add()["grows"] == 1
            R._assert_rows(U.read(), s, 0, s.n, names, "after update, move, remove and a growing add")
            with pytest.raises(pkg.GsrError):                       # refused: the cloud has SH and the new rows have none
                U.add(M._cloud(pkg, 15, sh=False, n=50))
            assert U.read_info()["n_splats"] == s.n
            U.upload(small)
            U.render(cam)
            live = E.live_handles()
            assert all(l > b for l, b in zip(live, base)), (live, base)
        assert E.live_handles() == base
        # ... and a context that never held anything
        with pkg.Engine(0):
            assert all(l > b for l, b in zip(E.live_handles(), base))
        assert E.live_handles() == base
    finally:
        hb.free()
