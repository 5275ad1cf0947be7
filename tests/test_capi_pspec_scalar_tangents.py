"""The C entries of K tangent pairs with a scalar (nns_spec_ns_scalar_tangents_workspace, nns_spec_ns_step_scalar_tangents_f32,
nns_spec_ns_tangent_variance_gram_f64) refuse bad arguments in the order include/nns.h states, before any launch: no GPU is needed, and none
is used -- every call below must return from its argument checks (a launch or a device query would fail or fault on the host pointers).
Fails where the symbols are missing."""
import ctypes
import os

import numpy as np

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
TWO_PI = 2 * np.pi


def _lib():
    from nns import _lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.lib()


def test_the_symbols_are_bound():
    from nns import _lib as L
    names = ('nns_spec_ns_scalar_tangents_workspace', 'nns_spec_ns_step_scalar_tangents_f32', 'nns_spec_ns_tangent_variance_gram_f64')
    bound = dict(L._SINGLE) if hasattr(L, '_SINGLE') else {}
    lib = _lib()
    for n in names:
        assert n in bound, n
        assert getattr(lib, n).argtypes is not None and len(getattr(lib, n).argtypes) == len(bound[n]), n


def test_workspace_query_formula_and_refusals():
    L = _lib()
    n, one = ctypes.c_size_t(0), ctypes.c_size_t(0)
    for B, K, nx, ny in ((1, 3, 64, 64), (2, 8, 128, 512), (3, 32, 64, 64), (1, 1, 1024, 64)):
        assert L.nns_spec_ns_scalar_tangents_workspace(B, K, nx, ny, ctypes.byref(n)) == 0
        assert L.nns_spec_ns_workspace(B, nx, ny, ctypes.byref(one)) == 0
        my1 = (ny - 1) // 3 + 1
        assert n.value == max((10 + 10 * K) * B * nx * my1 * 8, one.value), (B, K, nx, ny)
    assert L.nns_spec_ns_scalar_tangents_workspace(2, 1, 64, 64, ctypes.byref(n)) == 0
    assert L.nns_spec_ns_scalar_tangent_workspace(2, 64, 64, ctypes.byref(one)) == 0 and n.value == one.value      # K = 1 is the scalar tangent's
    assert L.nns_spec_ns_scalar_tangents_workspace(2, 3, 64, 64, None) == INVALID
    assert L.nns_spec_ns_scalar_tangents_workspace(0, 3, 64, 64, ctypes.byref(n)) == INVALID
    assert L.nns_spec_ns_scalar_tangents_workspace(2, 0, 64, 64, ctypes.byref(n)) == INVALID and b'ntan' in L.nns_last_error()
    assert L.nns_spec_ns_scalar_tangents_workspace(2, 33, 64, 64, ctypes.byref(n)) == INVALID and b'ntan' in L.nns_last_error()
    assert L.nns_spec_ns_scalar_tangents_workspace(2, 3, 96, 64, ctypes.byref(n)) == UNSUPPORTED


def test_the_step_refuses_in_the_stated_order_before_any_launch():
    L = _lib()
    need = ctypes.c_size_t(0)
    assert L.nns_spec_ns_scalar_tangents_workspace(2, 3, 64, 64, ctypes.byref(need)) == 0
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)                          # a host pointer: only ever compared with NULL
    call = L.nns_spec_ns_step_scalar_tangents_f32

    def args(what=p, that=p, dwhat=p, dthat=p, ntan=3, mean=p, ghat=None, gbatch=0, work=p, nbytes=need.value, batch=2, nx=64, Lx=TWO_PI, dt=0.01,
             nu=1e-3, drag=0.1, kappa=1e-3, gx=0.0, bx=0.0, lin=None, amp=None, clock=None, ids=None, nsteps=1):
        return (what, that, dwhat, dthat, ntan, mean, ghat, gbatch, work, nbytes, batch, nx, 64, Lx, TWO_PI, dt, nu, drag, kappa, gx, 0.0, bx, 0.0,
                lin, amp, 0, clock, ids, nsteps, None)
    err = lambda: L.nns_last_error()
    # 1. a NULL that / dwhat / dthat, before ntan is looked at
    for name in ('that', 'dwhat', 'dthat'):
        assert call(*args(ntan=0, **{name: None})) == INVALID and b'that, dwhat and dthat' in err(), name
    # 2. ntan outside [1, 32], before the forward call's own checks (a NULL what, a bad dt, a bad axis and a small workspace ride along)
    for ntan in (0, -1, 33):
        assert call(*args(ntan=ntan, what=None, dt=-1.0, nx=96, nbytes=0)) == INVALID and b'ntan' in err(), ntan
    # 3. the forward call's errors, before the workspace
    assert call(*args(amp=p, nbytes=0)) == INVALID and b'amp, clock and ids' in err()
    assert call(*args(amp=p, clock=p, nbytes=0)) == INVALID
    assert call(*args(what=None, nbytes=0)) == INVALID
    assert call(*args(mean=None, nbytes=0)) == INVALID and call(*args(work=None, nbytes=0)) == INVALID and call(*args(batch=0, nbytes=0)) == INVALID
    assert call(*args(dt=0.0, nbytes=0)) == INVALID and call(*args(nu=-1.0, nbytes=0)) == INVALID and call(*args(nsteps=-1, nbytes=0)) == INVALID
    assert call(*args(drag=-0.1, nbytes=0)) == INVALID and b'drag' in err()
    assert call(*args(kappa=-1.0, nbytes=0)) == INVALID and b'kappa' in err()
    assert call(*args(gx=float('inf'), nbytes=0)) == INVALID
    assert call(*args(bx=float('nan'), nbytes=0)) == INVALID and b'buoyancy' in err()
    assert call(*args(ghat=p, gbatch=3, nbytes=0)) == INVALID and b'gbatch' in err()
    assert call(*args(ghat=None, gbatch=1, nbytes=0)) == INVALID
    assert call(*args(Lx=-1.0, nbytes=0)) == INVALID
    assert call(*args(nx=96, nbytes=0)) == UNSUPPORTED
    # 4. the workspace last
    assert call(*args(nbytes=need.value - 1)) == WORKSPACE and b'nns_spec_ns_scalar_tangents_workspace' in err()
    smaller = ctypes.c_size_t(0)
    assert L.nns_spec_ns_scalar_tangents_workspace(2, 2, 64, 64, ctypes.byref(smaller)) == 0 and smaller.value < need.value
    assert call(*args(nbytes=smaller.value)) == WORKSPACE              # the workspace of fewer members does not serve
    # nothing to do is not an error, and launches nothing
    assert call(*args(nsteps=0)) == 0
    assert all(v == 0.0 for v in buf)


def test_the_variance_gram_refuses_before_any_launch():
    L = _lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    call = L.nns_spec_ns_tangent_variance_gram_f64
    assert call(None, 3, p, 2, 64, 64, None) == INVALID and call(p, 3, None, 2, 64, 64, None) == INVALID
    assert call(p, 3, p, 0, 64, 64, None) == INVALID
    assert call(p, 0, p, 2, 64, 64, None) == INVALID and b'ntan' in L.nns_last_error()
    assert call(p, 33, p, 2, 64, 64, None) == INVALID and b'ntan' in L.nns_last_error()
    assert call(p, 3, p, 2, 96, 64, None) == UNSUPPORTED and call(p, 3, p, 2, 64, 2048, None) == UNSUPPORTED
    assert all(v == 0.0 for v in buf)
