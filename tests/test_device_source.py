"""Device sources without a GPU: the C ABI refuses a NULL context, the ctypes mirror of gsr_device_attrs has the header's layout, and
device_attrs_struct takes device pointers and torch-like tensors apart before anything reaches the library."""
import ctypes as C

import pytest

GSR_E_INVALID = -1


def test_verbs_refuse_a_null_context(pkg):
    E = pkg.engine
    L = pkg.load_library()
    a = E.gsr_device_attrs()
    assert L.gsr_upload_append_device(None, 1, C.byref(a)) == GSR_E_INVALID
    assert L.gsr_update_device(None, 0, 1, C.byref(a)) == GSR_E_INVALID
    assert L.gsr_move_device(None, 0, 1, None, C.byref(a)) == GSR_E_INVALID
    assert L.gsr_debug_check_device_source(None, C.c_void_p(4096), 4) == GSR_E_INVALID
    assert b"gsr_debug_check_device_source" in L.gsr_last_error()


def test_struct_layout(pkg):
    S = pkg.engine.gsr_device_attrs
    assert C.sizeof(S) == 56
    names = ("P", "Cd", "alpha", "scale", "orient", "sh", "sh_vec3_per_point", "reserved_")
    assert [n for n, _ in S._fields_] == list(names)
    assert [getattr(S, n).offset for n in names] == [0, 8, 16, 24, 32, 40, 48, 52]


def test_struct_from_plain_ints(pkg):
    E = pkg.engine
    a, n, keep = E.device_attrs_struct(n=10, Cd=0x1000, alpha=0x2000, sh=0x3000, sh_vec3_per_point=15)
    assert (n, keep) == (10, [])
    assert (a.P, a.Cd, a.alpha, a.scale, a.orient, a.sh) == (None, 0x1000, 0x2000, None, None, 0x3000)
    assert (a.sh_vec3_per_point, a.reserved_) == (15, 0)
    a, n, _ = E.device_attrs_struct()
    assert n == 0 and not any((a.P, a.Cd, a.alpha, a.scale, a.orient, a.sh))
    with pytest.raises(E.GsrError) as ei:
        E.device_attrs_struct(Cd=0x1000)                             # an int pointer says nothing about n
    assert ei.value.code == -1
    with pytest.raises(E.GsrError):
        E.device_attrs_struct(n=10, sh=0x3000)                       # ... nor about the vec3 per point
    with pytest.raises(E.GsrError):
        E.device_attrs_struct(n=10, shx=0x3000)                      # the half verbs' names are not this struct's


class _FakeDeviceTensor:
    """what device_attrs_struct asks of a tensor, for the accepting path (this box has no GPU to put a real one on)"""
    dtype = "torch.float32"
    is_cuda = True

    def __init__(self, *shape, ptr=0x7f0000001000):
        self.shape, self.ptr = shape, ptr

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return self.ptr


def test_struct_from_tensor_like_objects(pkg):
    E = pkg.engine
    T = _FakeDeviceTensor
    cd, al, sh = T(7, 3, ptr=0x1000), T(7, ptr=0x2000), T(7, 15, 3, ptr=0x3000)
    a, n, keep = E.device_attrs_struct(Cd=cd, alpha=al, sh=sh)
    assert n == 7 and keep == [cd, al, sh] and (a.Cd, a.alpha, a.sh, a.sh_vec3_per_point) == (0x1000, 0x2000, 0x3000, 15)
    assert E.device_attrs_struct(n=7, alpha=T(7, 1))[1] == 7
    for bad in (dict(Cd=cd, alpha=T(8)), dict(n=6, Cd=cd), dict(Cd=T(7, 4)), dict(sh=T(7, 15, 2)), dict(sh=sh, sh_vec3_per_point=16), dict(alpha=T())):
        with pytest.raises(E.GsrError) as ei:
            E.device_attrs_struct(**bad)
        assert ei.value.code == -1, bad


def test_struct_refuses_tensors_the_gpu_cannot_read(pkg):
    torch = pytest.importorskip("torch")
    E = pkg.engine
    ok = torch.zeros((6, 3), dtype=torch.float32)
    cases = {
        "a CPU tensor": dict(Cd=ok),
        "float64": dict(Cd=torch.zeros((6, 3), dtype=torch.float64)),
        "not contiguous": dict(Cd=torch.zeros((3, 6), dtype=torch.float32).t()),
    }
    for label, kw in cases.items():
        with pytest.raises(E.GsrError) as ei:
            E.device_attrs_struct(**kw)
        assert ei.value.code == -1, label
    # (row counts that disagree need tensors that pass these checks first: test_struct_from_tensor_like_objects.)
    # The reasons are the ones named: dtype and layout are looked at before the device
    with pytest.raises(E.GsrError, match="float32"):
        E.device_attrs_struct(**cases["float64"])
    with pytest.raises(E.GsrError, match="contiguous"):
        E.device_attrs_struct(**cases["not contiguous"])
    with pytest.raises(E.GsrError, match="not on a GPU"):
        E.device_attrs_struct(**cases["a CPU tensor"])
