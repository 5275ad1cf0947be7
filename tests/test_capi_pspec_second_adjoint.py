"""The C entries of the second-order adjoint (nns_spec_ns_second_adjoint_workspace, nns_spec_ns_step_second_adjoint_f32) refuse bad arguments
in the order include/nns.h states, before any launch: no GPU is needed, and none is used -- every call below must return from its argument
checks (a launch or a device query would fail or fault on the host pointers).  Fails where the symbols are missing."""
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
    from nns import ops
    names = ('nns_spec_ns_second_adjoint_workspace', 'nns_spec_ns_step_second_adjoint_f32')
    bound = dict(L._SINGLE) if hasattr(L, '_SINGLE') else {}
    lib = _lib()
    for n in names:
        assert n in bound, n
        assert getattr(lib, n).argtypes is not None and len(getattr(lib, n).argtypes) == len(bound[n]), n
    assert len(bound['nns_spec_ns_step_second_adjoint_f32']) == 24
    assert callable(ops.spec_ns_second_adjoint_workspace) and callable(ops.spec_ns_second_adjoint_)


def test_workspace_query_formula_and_refusals():
    L = _lib()
    n, other = ctypes.c_size_t(0), ctypes.c_size_t(0)
    for B, nx, ny in ((1, 64, 64), (2, 128, 512), (3, 64, 64), (1, 1024, 64), (2, 64, 1024)):
        assert L.nns_spec_ns_second_adjoint_workspace(B, nx, ny, ctypes.byref(n)) == 0
        assert L.nns_spec_ns_workspace(B, nx, ny, ctypes.byref(other)) == 0
        my1 = (ny - 1) // 3 + 1
        assert n.value == max(24 * B * nx * my1 * 8, other.value), (B, nx, ny)
        for query in (L.nns_spec_ns_adjoint_workspace, L.nns_spec_ns_tangent_workspace):         # it serves the calls it is made of
            assert query(B, nx, ny, ctypes.byref(other)) == 0 and n.value >= other.value
    assert L.nns_spec_ns_second_adjoint_workspace(2, 64, 64, None) == INVALID
    assert L.nns_spec_ns_second_adjoint_workspace(0, 64, 64, ctypes.byref(n)) == INVALID
    assert L.nns_spec_ns_second_adjoint_workspace(2, 96, 64, ctypes.byref(n)) == UNSUPPORTED
    assert L.nns_spec_ns_second_adjoint_workspace(2, 64, 2048, ctypes.byref(n)) == UNSUPPORTED


def test_the_step_refuses_in_the_stated_order_before_any_launch():
    L = _lib()
    need = ctypes.c_size_t(0)
    assert L.nns_spec_ns_second_adjoint_workspace(2, 64, 64, ctypes.byref(need)) == 0
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)                          # a host pointer: only ever compared with NULL
    call = L.nns_spec_ns_step_second_adjoint_f32

    def args(what0=p, dwhat0=p, mean=p, ghat=None, gbatch=0, dghat=None, dgbatch=0, lam=p, dlam=p, gbar=None, dgbar=None, work=p,
             nbytes=need.value, batch=2, nx=64, Lx=TWO_PI, dt=0.01, nu=1e-3, drag=0.1, lin=None, nsteps=1):
        return (what0, dwhat0, mean, ghat, gbatch, dghat, dgbatch, lam, dlam, gbar, dgbar, work, nbytes, batch, nx, 64, Lx, TWO_PI, dt, nu, drag,
                lin, nsteps, None)
    err = lambda: L.nns_last_error()
    # 1. the adjoint's NULL pointers and batch, before dwhat0 and dlam are looked at
    for name in ('what0', 'mean', 'lam', 'work'):
        assert call(*args(dwhat0=None, dlam=None, **{name: None})) == INVALID and b'NULL pointer or batch' in err(), name
    assert call(*args(dwhat0=None, batch=0)) == INVALID and b'NULL pointer or batch' in err()
    # 2. a NULL dwhat0 / dlam, before the numbers (a bad dt, a bad axis and a small workspace ride along)
    for name in ('dwhat0', 'dlam'):
        assert call(*args(dt=-1.0, nx=96, nbytes=0, **{name: None})) == INVALID and b'dwhat0 and dlam' in err(), name
    # 3. the numbers, before gbatch
    assert call(*args(dt=0.0, gbatch=1, nbytes=0)) == INVALID and b'dt' in err()
    assert call(*args(nu=-1.0, gbatch=1, nbytes=0)) == INVALID and b'nu' in err()
    assert call(*args(nsteps=-1, nbytes=0)) == INVALID
    assert call(*args(drag=-0.1, gbatch=1, nbytes=0)) == INVALID and b'drag' in err()
    # with a table nu and drag are not read: the next refusal is the workspace's
    assert call(*args(nu=-1.0, drag=-1.0, lin=p, nbytes=0)) == WORKSPACE
    # 4. gbatch, before dgbatch
    assert call(*args(ghat=p, gbatch=3, dgbatch=1, nbytes=0)) == INVALID and b' gbatch' in err()
    assert call(*args(ghat=None, gbatch=1, dgbatch=1, nbytes=0)) == INVALID and b' gbatch' in err()
    # 5. dgbatch, before the box
    assert call(*args(dgbatch=1, Lx=-1.0, nbytes=0)) == INVALID and b'dgbatch' in err()
    assert call(*args(dghat=p, dgbatch=0, nx=96, nbytes=0)) == INVALID and b'dgbatch' in err()
    assert call(*args(dghat=p, dgbatch=3, nbytes=0)) == INVALID and b'dgbatch' in err()
    # 6. the box and the axes, before the workspace
    assert call(*args(Lx=-1.0, nbytes=0)) == INVALID
    assert call(*args(nx=96, nbytes=0)) == UNSUPPORTED
    # 7. the workspace last
    assert call(*args(nbytes=need.value - 1)) == WORKSPACE and b'nns_spec_ns_second_adjoint_workspace' in err()
    smaller = ctypes.c_size_t(0)
    assert L.nns_spec_ns_adjoint_workspace(2, 64, 64, ctypes.byref(smaller)) == 0 and smaller.value < need.value
    assert call(*args(nbytes=smaller.value)) == WORKSPACE              # the first-order adjoint's workspace does not serve
    # nothing to do and nothing to zero is not an error, and launches nothing
    assert call(*args(nsteps=0)) == 0
    assert all(v == 0.0 for v in buf)
