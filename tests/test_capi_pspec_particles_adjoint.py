"""The C entries of the reverse mode of particle sampling (nns_spec_ns_particle_cells_i32, _spread_workspace, _spread_f32, _sample_grad_f32,
_coefs_adjoint_f32) are bound with the arity of include/nns.h and refuse bad arguments in the order it states, before any launch: no GPU
is needed, and none is used -- every call below must return from its argument checks (a launch would fail or fault on the host pointers,
which are only ever compared with NULL).  Fails where the symbols are missing."""
import ctypes
import os

import numpy as np

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
TWO_PI = 2 * np.pi
NAMES = ('nns_spec_ns_particle_cells_i32', 'nns_spec_ns_particle_spread_workspace', 'nns_spec_ns_particle_spread_f32',
         'nns_spec_ns_particle_sample_grad_f32', 'nns_spec_ns_particle_coefs_adjoint_f32')


def _lib():
    from nns import _lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.lib()


def _host_pointer():
    buf = (ctypes.c_float * 16)()
    return buf, ctypes.addressof(buf)                  # a host pointer: only ever compared with NULL


def test_the_symbols_are_bound():
    from nns import _lib as L
    from nns import ops
    from nns.periodic import PeriodicSolver
    bound = dict(L._SINGLE)
    lib = _lib()
    for n, arity in zip(NAMES, (9, 4, 16, 12, 13)):
        assert n in bound, n
        assert len(getattr(lib, n).argtypes) == len(bound[n]) == arity, n
    for f in ('spec_ns_particle_cells', 'spec_ns_particle_spread_workspace', 'spec_ns_particle_spread', 'spec_ns_particle_sample_grad',
              'spec_ns_particle_coefs_adjoint'):
        assert callable(getattr(ops, f)), f
    for m in ('observe', 'sample_gradient', 'spread', 'particle_cells'):
        assert callable(getattr(PeriodicSolver, m)), m


def test_the_header_declares_the_entries_with_that_arity():
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(here, '..', 'include', 'nns.h')).read()
    for n, arity in zip(NAMES, (9, 4, 16, 12, 13)):
        at = text.index('int %s(' % n)
        args = text[at:text.index(');', at)].split('(', 1)[1]
        assert len(args.split(',')) == arity, n


def test_spread_workspace_formula_and_refusals():
    L = _lib()
    n = ctypes.c_size_t(0)
    q = L.nns_spec_ns_particle_spread_workspace
    for B, P, order in ((1, 1, 4), (3, 257, 6), (8, 1 << 20, 4), (64, 65536, 6)):
        assert q(B, P, order, ctypes.byref(n)) == 0
        assert n.value == B * P * (2 * order + 4) * 4, (B, P, order)
    assert q(2, 10, 4, None) == INVALID
    assert q(0, 0, 5, ctypes.byref(n)) == INVALID and b'batch' in L.nns_last_error()
    assert q(2, 0, 5, ctypes.byref(n)) == INVALID and b'npart' in L.nns_last_error()
    assert q(2, 2 ** 30, 5, ctypes.byref(n)) == INVALID and b'npart' in L.nns_last_error()
    assert q(2, 10, 5, ctypes.byref(n)) == INVALID and b'order' in L.nns_last_error()


def test_cells_refuses_in_the_stated_order_before_any_launch():
    L = _lib()
    buf, p = _host_pointer()
    err = L.nns_last_error

    def call(pos=p, key=p, batch=2, npart=257, nx=64, ny=64, Lx=TWO_PI):
        return L.nns_spec_ns_particle_cells_i32(pos, key, batch, npart, nx, ny, Lx, TWO_PI, None)
    for name in ('pos', 'key'):
        assert call(npart=0, Lx=-1.0, nx=96, **{name: None}) == INVALID and b'NULL pointer or batch' in err(), name
    assert call(batch=0, npart=0) == INVALID and b'NULL pointer or batch' in err()
    for npart in (0, -1, 2 ** 30, 2 ** 40):
        assert call(npart=npart, Lx=-1.0, nx=96) == INVALID and b'npart' in err(), npart
    for Lx in (-1.0, 0.0, float('inf'), float('nan')):
        assert call(Lx=Lx, nx=96) == INVALID and b'Lx' in err()
    assert call(nx=96) == UNSUPPORTED and call(nx=2048) == UNSUPPORTED
    # batch nx ny >= 2^31: the keys are int32
    assert call(batch=2048, npart=1, nx=1024, ny=1024) == UNSUPPORTED and b'2^31' in err()
    assert call(batch=2048, npart=1, nx=96, ny=1024) == UNSUPPORTED and b'power of two' in err()
    assert all(v == 0.0 for v in buf)


def test_spread_refuses_in_the_stated_order_before_any_launch():
    L = _lib()
    need = ctypes.c_size_t(0)
    assert L.nns_spec_ns_particle_spread_workspace(2, 257, 4, ctypes.byref(need)) == 0
    buf, p = _host_pointer()
    err = L.nns_last_error

    def call(cot=p, pos=p, perm=p, start=p, cbar=p, nfields=2, order=4, work=p, nbytes=need.value, batch=2, npart=257, nx=64, ny=64, Lx=TWO_PI):
        return L.nns_spec_ns_particle_spread_f32(cot, pos, perm, start, cbar, nfields, order, work, nbytes, batch, npart, nx, ny, Lx, TWO_PI, None)
    # 1. NULL pointers and the batch (everything later rides along, wrong)
    for name in ('cot', 'pos', 'perm', 'start', 'cbar', 'work'):
        assert call(npart=0, order=5, nfields=0, Lx=-1.0, nx=96, nbytes=0, **{name: None}) == INVALID and b'NULL pointer or batch' in err(), name
    assert call(batch=0, npart=0) == INVALID and b'NULL pointer or batch' in err()
    # 2. particles  3. order  4. nfields  5. box  6. axes  7. workspace
    for npart in (0, -1, 2 ** 30):
        assert call(npart=npart, order=5, nfields=0, Lx=-1.0, nx=96, nbytes=0) == INVALID and b'npart' in err(), npart
    for order in (0, 3, 5, 8):
        assert call(order=order, nfields=0, Lx=-1.0, nx=96, nbytes=0) == INVALID and b'order' in err()
    for nfields in (0, 5):
        assert call(nfields=nfields, Lx=-1.0, nx=96, nbytes=0) == INVALID and b'nfields' in err()
    assert call(Lx=-1.0, nx=96, nbytes=0) == INVALID and b'Lx' in err()
    assert call(nx=96, nbytes=0) == UNSUPPORTED and b'power of two' in err()
    assert call(batch=2048, npart=1, nx=1024, ny=1024, nbytes=0) == UNSUPPORTED and b'2^31' in err()
    assert call(nbytes=need.value - 1) == WORKSPACE and b'nns_spec_ns_particle_spread_workspace' in err()
    assert call(order=6) == WORKSPACE                                   # the record grows with the order
    assert all(v == 0.0 for v in buf)


def test_sample_grad_refuses_in_the_stated_order_before_any_launch():
    L = _lib()
    buf, p = _host_pointer()
    err = L.nns_last_error

    def call(coef=p, pos=p, grad=p, nfields=2, order=4, batch=2, npart=257, nx=64, Lx=TWO_PI):
        return L.nns_spec_ns_particle_sample_grad_f32(coef, pos, grad, nfields, order, batch, npart, nx, 64, Lx, TWO_PI, None)
    for name in ('coef', 'pos', 'grad'):
        assert call(npart=0, order=5, **{name: None}) == INVALID and b'NULL pointer or batch' in err(), name
    assert call(batch=0, npart=0) == INVALID and b'NULL pointer or batch' in err()
    for npart in (0, -1, 2 ** 30, 2 ** 40):
        assert call(npart=npart, order=5, nfields=0) == INVALID and b'npart' in err(), npart
    assert call(order=5, nfields=0, Lx=-1.0) == INVALID and b'order' in err()
    for nfields in (0, 5):
        assert call(nfields=nfields, Lx=-1.0, nx=96) == INVALID and b'nfields' in err()
    assert call(Lx=-1.0, nx=96) == INVALID and b'Lx' in err()
    assert call(nx=96) == UNSUPPORTED
    assert all(v == 0.0 for v in buf)


def test_coefs_adjoint_refuses_in_the_stated_order_before_any_launch():
    L = _lib()
    need = ctypes.c_size_t(0)
    assert L.nns_spec_ns_particle_workspace(2, 2, 64, 64, ctypes.byref(need)) == 0
    buf, p = _host_pointer()
    err = L.nns_last_error

    def call(cbar=p, wbar=p, thbar=None, fields=3, order=4, work=p, nbytes=need.value, batch=2, nx=64, Lx=TWO_PI):
        return L.nns_spec_ns_particle_coefs_adjoint_f32(cbar, wbar, thbar, fields, order, work, nbytes, batch, nx, 64, Lx, TWO_PI, None)
    for name in ('cbar', 'work'):
        assert call(order=5, fields=0, Lx=-1.0, nx=96, nbytes=0, **{name: None}) == INVALID and b'NULL pointer or batch' in err(), name
    assert call(batch=0, order=5) == INVALID and b'NULL pointer or batch' in err()
    for order in (0, 3, 5, 8):
        assert call(order=order, fields=0, Lx=-1.0, nbytes=0) == INVALID and b'order' in err()
    for fields in (0, 16, -1):
        assert call(fields=fields, Lx=-1.0, nbytes=0) == INVALID and b'mask' in err()
    assert call(wbar=None, Lx=-1.0, nbytes=0) == INVALID and b'wbar_hat' in err()
    assert call(fields=8, Lx=-1.0, nbytes=0) == INVALID and b'theta' in err()
    assert call(fields=15, nx=96, nbytes=0) == INVALID and b'theta' in err()
    for Lx in (-1.0, 0.0, float('inf'), float('nan')):
        assert call(Lx=Lx, nx=96, nbytes=0) == INVALID and b'Lx' in err()
    assert call(nx=96, nbytes=0) == UNSUPPORTED and call(nx=2048, nbytes=0) == UNSUPPORTED
    assert call(nbytes=need.value - 1) == WORKSPACE and b'nns_spec_ns_particle_workspace' in err()
    assert call(fields=15, thbar=p) == WORKSPACE
    assert call(fields=8, wbar=None, thbar=p, nbytes=need.value // 2 - 1) == WORKSPACE          # theta alone needs no wbar_hat
    assert all(v == 0.0 for v in buf)
