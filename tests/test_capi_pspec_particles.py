"""The C entries of the Lagrangian tracers (nns_spec_ns_particle_workspace, _coefs_f32, _sample_f32, _stage_f32) are bound with the arity of
include/nns.h and refuse bad arguments in the order it states, before any launch: no GPU is needed, and none is used -- every call below must
return from its argument checks (a launch would fail or fault on the host pointers).  Fails where the symbols are missing."""
import ctypes
import os

import numpy as np

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
TWO_PI = 2 * np.pi
NAMES = ('nns_spec_ns_particle_workspace', 'nns_spec_ns_particle_coefs_f32', 'nns_spec_ns_particle_sample_f32', 'nns_spec_ns_particle_stage_f32')


def _lib():
    from nns import _lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.lib()


def test_the_symbols_are_bound():
    from nns import _lib as L
    from nns import ops
    bound = dict(L._SINGLE)
    lib = _lib()
    for n, arity in zip(NAMES, (5, 14, 12, 18)):
        assert n in bound, n
        assert len(getattr(lib, n).argtypes) == len(bound[n]) == arity, n
    for f in ('spec_ns_particle_workspace', 'spec_ns_particle_coefs', 'spec_ns_particle_sample', 'spec_ns_particle_stage_'):
        assert callable(getattr(ops, f)), f


def test_workspace_query_formula_and_refusals():
    L = _lib()
    n = ctypes.c_size_t(0)
    for B, nf, nx, ny in ((1, 1, 64, 64), (3, 2, 64, 128), (2, 4, 1024, 64), (8, 2, 1024, 1024)):
        assert L.nns_spec_ns_particle_workspace(B, nf, nx, ny, ctypes.byref(n)) == 0
        assert n.value == nf * B * nx * (ny // 2 + 1) * 8, (B, nf, nx, ny)
    q = L.nns_spec_ns_particle_workspace
    assert q(2, 2, 64, 64, None) == INVALID
    assert q(0, 0, 96, 64, ctypes.byref(n)) == INVALID and b'batch' in L.nns_last_error()
    assert q(2, 0, 96, 64, ctypes.byref(n)) == INVALID and b'nfields' in L.nns_last_error()
    assert q(2, 5, 64, 64, ctypes.byref(n)) == INVALID
    assert q(2, 2, 96, 64, ctypes.byref(n)) == UNSUPPORTED
    assert q(2, 2, 64, 2048, ctypes.byref(n)) == UNSUPPORTED


def _host_pointer():
    buf = (ctypes.c_float * 16)()
    return buf, ctypes.addressof(buf)                  # a host pointer: only ever compared with NULL


def test_coefs_refuses_in_the_stated_order_before_any_launch():
    L = _lib()
    need = ctypes.c_size_t(0)
    assert L.nns_spec_ns_particle_workspace(2, 2, 64, 64, ctypes.byref(need)) == 0
    buf, p = _host_pointer()
    err = L.nns_last_error

    def call(what=p, that=None, mean=p, coef=p, fields=3, order=4, work=p, nbytes=need.value, batch=2, nx=64, Lx=TWO_PI):
        return L.nns_spec_ns_particle_coefs_f32(what, that, mean, coef, fields, order, work, nbytes, batch, nx, 64, Lx, TWO_PI, None)
    # 1. NULL pointers and the batch, before the order (a bad order, mask, box, axis and workspace ride along)
    for name in ('what', 'mean', 'coef', 'work'):
        assert call(order=5, fields=0, Lx=-1.0, nx=96, nbytes=0, **{name: None}) == INVALID and b'NULL pointer or batch' in err(), name
    assert call(batch=0, order=5) == INVALID and b'NULL pointer or batch' in err()
    # 2. the order, before the mask
    for order in (0, 3, 5, 8):
        assert call(order=order, fields=0, Lx=-1.0, nbytes=0) == INVALID and b'order' in err()
    # 3. an empty or overlong mask, then theta without that, before the box
    for fields in (0, 16, -1):
        assert call(fields=fields, Lx=-1.0, nbytes=0) == INVALID and b'mask' in err()
    assert call(fields=8, Lx=-1.0, nbytes=0) == INVALID and b'theta' in err()
    assert call(fields=15, nx=96, nbytes=0) == INVALID and b'theta' in err()
    # 4. the box lengths, before the axes
    for Lx in (-1.0, 0.0, float('inf'), float('nan')):
        assert call(Lx=Lx, nx=96, nbytes=0) == INVALID and b'Lx' in err()
    # 5. the axes, before the workspace
    assert call(nx=96, nbytes=0) == UNSUPPORTED
    assert call(nx=2048, nbytes=0) == UNSUPPORTED
    # 6. the workspace last: it grows with the number of fields asked for
    assert call(nbytes=need.value - 1) == WORKSPACE and b'nns_spec_ns_particle_workspace' in err()
    assert call(fields=15, that=p) == WORKSPACE
    assert call(fields=4, nbytes=need.value // 2 - 1) == WORKSPACE
    assert all(v == 0.0 for v in buf)


def test_sample_refuses_in_the_stated_order_before_any_launch():
    L = _lib()
    buf, p = _host_pointer()
    err = L.nns_last_error

    def call(coef=p, pos=p, out=p, nfields=2, order=4, batch=2, npart=257, nx=64, Lx=TWO_PI):
        return L.nns_spec_ns_particle_sample_f32(coef, pos, out, nfields, order, batch, npart, nx, 64, Lx, TWO_PI, None)
    for name in ('coef', 'pos', 'out'):
        assert call(npart=0, order=5, **{name: None}) == INVALID and b'NULL pointer or batch' in err(), name
    assert call(batch=0, npart=0) == INVALID and b'NULL pointer or batch' in err()
    # the particle count, before the order
    for npart in (0, -1, 2 ** 30, 2 ** 40):
        assert call(npart=npart, order=5, nfields=0) == INVALID and b'npart' in err(), npart
    assert call(order=5, nfields=0, Lx=-1.0) == INVALID and b'order' in err()
    for nfields in (0, 5):
        assert call(nfields=nfields, Lx=-1.0, nx=96) == INVALID and b'nfields' in err()
    assert call(Lx=-1.0, nx=96) == INVALID and b'Lx' in err()
    assert call(nx=96) == UNSUPPORTED
    assert all(v == 0.0 for v in buf)


def test_stage_refuses_in_the_stated_order_before_any_launch():
    L = _lib()
    buf, p = _host_pointer()
    other = ctypes.addressof(buf) + 8
    err = L.nns_last_error

    def call(coef=p, pos0=p, pos_in=p, pos_out=other, acc=p, a=0.1, wk=1.0, c=0.0, first=0, closing=0, order=4, batch=2, npart=257, nx=64,
             Lx=TWO_PI):
        return L.nns_spec_ns_particle_stage_f32(coef, pos0, pos_in, pos_out, acc, a, wk, c, first, closing, order, batch, npart, nx, 64, Lx, TWO_PI,
                                                None)
    for name in ('coef', 'pos0', 'pos_in', 'pos_out'):
        assert call(acc=None, npart=0, **{name: None}) == INVALID and b'NULL pointer or batch' in err(), name
    assert call(batch=0, acc=None) == INVALID and b'NULL pointer or batch' in err()
    # a NULL acc serves only a stage that is both first and closing; then the aliasing of pos_out; both before the particle count
    for first, closing in ((0, 0), (1, 0), (0, 1)):
        assert call(acc=None, first=first, closing=closing, pos_out=p, npart=0) == INVALID and b'acc is NULL' in err()
    assert call(pos_out=p, npart=0) == INVALID and b'alias' in err()
    assert call(pos_out=p, first=1, npart=0) == INVALID and b'alias' in err()
    # the particle count, before the order; the order before the coefficients of the stage; those before the box
    assert call(npart=0, order=5) == INVALID and b'npart' in err()
    assert call(pos_out=p, closing=1, npart=2 ** 30, order=5) == INVALID and b'npart' in err()          # aliasing is fine in the closing stage
    assert call(acc=None, first=1, closing=1, npart=0) == INVALID and b'npart' in err()
    assert call(order=6 + 1, a=float('nan'), Lx=-1.0) == INVALID and b'order' in err()
    for name in ('a', 'wk', 'c'):
        assert call(Lx=-1.0, nx=96, **{name: float('inf')}) == INVALID and b'finite' in err() and b'Lx' not in err(), name
    assert call(Lx=0.0, nx=96) == INVALID and b'Lx' in err()
    assert call(nx=96) == UNSUPPORTED
    assert call(order=6, nx=32) == UNSUPPORTED
    assert all(v == 0.0 for v in buf)
