"""Which C entry every configuration of nns.periodic.PeriodicSolver reaches, and with which numbers: ``step`` and the reverse mode
(``evolve`` / ``advance``) are run under nns._lib.CallRecorder and the recorded nns_spec_ns_step* calls compared with the table below.  That
a plain solver calls nns_spec_ns_step_f32 and not a more general entry is what makes ``step`` bitwise the same from one version of the Python
layer to the next, and what keeps the name in the library's error messages.  64 x 64 (the smallest axis), B = 2: only the dispatch is under
test."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, B, DT, NU, NSTEPS = 64, 2, 0.01, 1e-3, 2
DRAG, KAPPA, GRAD, BUOY, SEED = 0.1, 2e-3, (0.3, -0.2), (0.0, 0.5), 7
TWO_PI = 2 * np.pi

BOX = 'work nbytes B nx ny Lx Ly dt'
ARGS = {name: layout.replace('BOX', BOX).split() for name, layout in {
    'nns_spec_ns_step_f32': 'what mean BOX nu nsteps stream',
    'nns_spec_ns_step_forced_f32': 'what mean ghat gbatch BOX nu drag nsteps stream',
    'nns_spec_ns_step_scalar_f32': 'what that mean ghat gbatch BOX nu drag kappa gx gy nsteps stream',
    'nns_spec_ns_step_buoyant_f32': 'what that mean ghat gbatch BOX nu drag kappa gx gy bx by nsteps stream',
    'nns_spec_ns_step_stochastic_f32': 'what that mean ghat gbatch BOX nu drag kappa gx gy bx by amp seed clock ids nsteps stream',
    'nns_spec_ns_step_linear_f32': 'what that mean ghat gbatch BOX kappa gx gy bx by lin amp seed clock ids nsteps stream',
    'nns_spec_ns_step_adjoint_f32': 'what0 mean ghat gbatch lam gbar BOX nu drag nsteps stream',
    'nns_spec_ns_step_scalar_adjoint_f32': 'what0 that0 mean ghat gbatch lam mu gbar BOX nu drag kappa gx gy bx by nsteps stream',
    'nns_spec_ns_step_linear_adjoint_f32': 'what0 that0 mean ghat gbatch lam mu gbar BOX kappa gx gy bx by lin nsteps stream',
    'nns_spec_ns_step_operator_adjoint_f32': 'what0 that0 mean ghat gbatch lam mu gbar BOX kappa gx gy bx by lin nsteps stream lbar',
}.items()}
POINTERS = ('what', 'that', 'mean', 'ghat', 'work', 'amp', 'clock', 'ids', 'lin', 'what0', 'that0', 'lam', 'mu', 'gbar', 'lbar')


def solver(ring=False, force=False, **kw):
    from nns.periodic import PeriodicSolver
    s = PeriodicSolver(N, N, DT, 1.0, NU, **kw)
    if force:
        s.kolmogorov_forcing()
    if ring:
        s.ring_forcing(1.0, 3.0, 5.0, seed=SEED)
    return s


def field(k, grad=False):
    g = torch.Generator().manual_seed(k)
    return torch.randn((B, N, N), generator=g).cuda().requires_grad_(grad)


def state(s, theta=False):
    return s.init(field(1), field(2), field(3) if theta else None)


def step_calls(run, key='calls'):
    """[(name, {argument: value})] of the nns_spec_ns_step* calls that run() makes, every argument list as long as its entry's."""
    from nns import _lib
    rec = _lib.CallRecorder()
    with rec.stage(key):
        run()
    out = []
    for f, args, name in rec.stages[key]:
        if '_step' in name:
            assert len(args) == len(ARGS[name]), name
            out.append((name, dict(zip(ARGS[name], args))))
    return out


def check_call(call, name, nsteps, null=(), **numbers):
    """One recorded call: its entry, the box, nsteps, the given doubles and ints, and which pointers are NULL (the others are not)."""
    got, a = call
    assert got == name
    want = dict(dict(nbytes=a['nbytes'], B=B, nx=N, ny=N, Lx=TWO_PI, Ly=TWO_PI, dt=DT, nsteps=nsteps), **numbers)
    numeric = {k: v for k, v in a.items() if k not in POINTERS and k != 'stream'}
    assert numeric == want                                # every double and int of the entry is named in the table, bit for bit
    assert a['nbytes'] > 0
    for k in POINTERS:
        if k in a:
            assert (a[k] is None) == (k in null), (name, k)


SCALAR = dict(kappa=KAPPA, scalar_gradient=GRAD)
FLOW0 = dict(kappa=0.0, gx=0.0, gy=0.0, bx=0.0, by=0.0)                      # what a solver without a scalar passes where the entry takes them
# id: (solver arguments, state with theta, entry, NULL pointers, numbers)
FORWARD = {
    'plain': (dict(), False, 'nns_spec_ns_step_f32', (), dict(nu=NU)),
    'drag': (dict(drag=DRAG), False, 'nns_spec_ns_step_forced_f32', ('ghat',), dict(nu=NU, drag=DRAG, gbatch=0)),
    'kolmogorov': (dict(force=True), False, 'nns_spec_ns_step_forced_f32', (), dict(nu=NU, drag=0.0, gbatch=1)),
    'kappa-no-theta': (dict(**SCALAR), False, 'nns_spec_ns_step_f32', (), dict(nu=NU)),
    'kappa-no-theta-drag': (dict(drag=DRAG, buoyancy=BUOY, **SCALAR), False, 'nns_spec_ns_step_forced_f32', ('ghat',),
                            dict(nu=NU, drag=DRAG, gbatch=0)),
    'scalar': (dict(**SCALAR), True, 'nns_spec_ns_step_scalar_f32', ('ghat',),
               dict(nu=NU, drag=0.0, kappa=KAPPA, gx=GRAD[0], gy=GRAD[1], gbatch=0)),
    'buoyant': (dict(buoyancy=BUOY, force=True, drag=DRAG, **SCALAR), True, 'nns_spec_ns_step_buoyant_f32', (),
                dict(nu=NU, drag=DRAG, kappa=KAPPA, gx=GRAD[0], gy=GRAD[1], bx=BUOY[0], by=BUOY[1], gbatch=1)),
    'stochastic-scalar': (dict(ring=True, buoyancy=BUOY, **SCALAR), True, 'nns_spec_ns_step_stochastic_f32', ('ghat',),
                          dict(nu=NU, drag=0.0, kappa=KAPPA, gx=GRAD[0], gy=GRAD[1], bx=BUOY[0], by=BUOY[1], seed=SEED, gbatch=0)),
    'stochastic': (dict(ring=True, drag=DRAG), False, 'nns_spec_ns_step_stochastic_f32', ('that', 'ghat'),
                   dict(FLOW0, nu=NU, drag=DRAG, seed=SEED, gbatch=0)),
    'stochastic-kappa-no-theta': (dict(ring=True, **SCALAR), False, 'nns_spec_ns_step_stochastic_f32', ('that', 'ghat'),
                                  dict(FLOW0, nu=NU, drag=0.0, kappa=KAPPA, gx=GRAD[0], gy=GRAD[1], seed=SEED, gbatch=0)),
    'beta': (dict(beta=1.0), False, 'nns_spec_ns_step_linear_f32', ('that', 'ghat', 'amp', 'clock', 'ids'), dict(FLOW0, seed=0, gbatch=0)),
    'beta-stochastic': (dict(beta=1.0, ring=True, force=True), False, 'nns_spec_ns_step_linear_f32', ('that',),
                        dict(FLOW0, seed=SEED, gbatch=1)),
    'hyperviscous-scalar': (dict(hyperviscosity=(1e-8, 2), buoyancy=BUOY, **SCALAR), True, 'nns_spec_ns_step_linear_f32',
                            ('ghat', 'amp', 'clock', 'ids'),
                            dict(kappa=KAPPA, gx=GRAD[0], gy=GRAD[1], bx=BUOY[0], by=BUOY[1], seed=0, gbatch=0)),
}


@pytest.mark.parametrize('case', sorted(FORWARD))
def test_step_makes_one_call_of_its_entry(gpu_device, case):
    kw, theta, name, null, numbers = FORWARD[case]
    s = solver(**kw)
    st = state(s, theta)
    calls = step_calls(lambda: s.step(st, NSTEPS))
    assert len(calls) == 1
    check_call(calls[0], name, NSTEPS, null, **numbers)
    assert st.steps == NSTEPS


@pytest.mark.parametrize('base', [dict(), dict(drag=DRAG), dict(force=True)])
def test_kappa_without_a_scalar_in_the_state_changes_no_call(gpu_device, base):
    calls = []
    for kw in (base, dict(base, **SCALAR)):
        s = solver(**kw)
        st = state(s)
        (name, a), = step_calls(lambda: s.step(st, NSTEPS))
        calls.append((name, {k: (v is None) if k in POINTERS else v for k, v in a.items() if k != 'stream'}))
    assert calls[0] == calls[1]


def backward_calls(s, run):
    """(forward, backward): the step calls of run(), which returns tensors, and of the backward of their sum."""
    out = []
    fwd = step_calls(lambda: out.append(run()), 'forward')
    total = sum(o.sum() for o in (out[0] if isinstance(out[0], tuple) else (out[0],)))
    bwd = step_calls(total.backward, 'backward')
    return fwd, bwd


def test_evolve_with_an_operator_takes_the_linear_step_one_step_per_call(gpu_device):
    s = solver()
    w = field(4)
    calls = step_calls(lambda: s.evolve(w, NSTEPS, operator=s.operator_table(device='cuda')))
    assert len(calls) == NSTEPS
    for call in calls:
        check_call(call, 'nns_spec_ns_step_linear_f32', 1, ('that', 'ghat', 'amp', 'clock', 'ids'), **dict(FLOW0, seed=0, gbatch=0))


FLOW_ADJ = ('nns_spec_ns_step_adjoint_f32', ('ghat', 'gbar'), dict(nu=NU, drag=0.0, gbatch=0))
SCALAR_NUMBERS = dict(kappa=KAPPA, gx=GRAD[0], gy=GRAD[1])
# id: (solver arguments, theta, operator: None / 'constant' / 'grad', forcing argument, forward entry, adjoint entry, NULL pointers, numbers)
BACKWARD = {
    'plain': (dict(), False, None, False, 'nns_spec_ns_step_f32') + FLOW_ADJ,
    'forced': (dict(force=True, drag=DRAG), False, None, False, 'nns_spec_ns_step_forced_f32', 'nns_spec_ns_step_adjoint_f32', ('gbar',),
               dict(nu=NU, drag=DRAG, gbatch=1)),
    'forcing-argument': (dict(), False, None, True, 'nns_spec_ns_step_forced_f32', 'nns_spec_ns_step_adjoint_f32', (),
                         dict(nu=NU, drag=0.0, gbatch=1)),
    'stochastic': (dict(ring=True), False, None, False, 'nns_spec_ns_step_stochastic_f32') + FLOW_ADJ,
    'scalar': (dict(**SCALAR), True, None, False, 'nns_spec_ns_step_scalar_f32', 'nns_spec_ns_step_scalar_adjoint_f32', ('ghat', 'gbar'),
               dict(SCALAR_NUMBERS, nu=NU, drag=0.0, bx=0.0, by=0.0, gbatch=0)),
    'buoyant': (dict(buoyancy=BUOY, drag=DRAG, **SCALAR), True, None, False, 'nns_spec_ns_step_buoyant_f32',
                'nns_spec_ns_step_scalar_adjoint_f32', ('ghat', 'gbar'),
                dict(SCALAR_NUMBERS, nu=NU, drag=DRAG, bx=BUOY[0], by=BUOY[1], gbatch=0)),
    'beta': (dict(beta=1.0), False, None, False, 'nns_spec_ns_step_linear_f32', 'nns_spec_ns_step_linear_adjoint_f32',
             ('that0', 'mu', 'ghat', 'gbar'), dict(FLOW0, gbatch=0)),
    'beta-stochastic': (dict(beta=1.0, ring=True), False, None, False, 'nns_spec_ns_step_linear_f32', 'nns_spec_ns_step_linear_adjoint_f32',
                        ('that0', 'mu', 'ghat', 'gbar'), dict(FLOW0, gbatch=0)),
    'beta-buoyant': (dict(beta=1.0, buoyancy=BUOY, **SCALAR), True, None, False, 'nns_spec_ns_step_linear_f32',
                     'nns_spec_ns_step_linear_adjoint_f32', ('ghat', 'gbar'), dict(SCALAR_NUMBERS, bx=BUOY[0], by=BUOY[1], gbatch=0)),
    'operator-constant': (dict(), False, 'constant', False, 'nns_spec_ns_step_linear_f32', 'nns_spec_ns_step_linear_adjoint_f32',
                          ('that0', 'mu', 'ghat', 'gbar'), dict(FLOW0, gbatch=0)),
    'operator-grad': (dict(), False, 'grad', False, 'nns_spec_ns_step_linear_f32', 'nns_spec_ns_step_operator_adjoint_f32',
                      ('that0', 'mu', 'ghat', 'gbar'), dict(FLOW0, gbatch=0)),
}


@pytest.mark.parametrize('case', sorted(BACKWARD))
def test_backward_makes_one_call_of_its_adjoint(gpu_device, case):
    kw, theta, operator, forcing, forward, name, null, numbers = BACKWARD[case]
    s = solver(**kw)
    w = field(4, grad=True)
    args = dict()
    if theta:
        args['theta'] = field(5, grad=True)
    if forcing:
        args['forcing'] = field(6, grad=True)[:1].detach().requires_grad_(True)
    if operator:
        args['operator'] = s.operator_table(device='cuda').requires_grad_(operator == 'grad')
    fwd, bwd = backward_calls(s, lambda: s.evolve(w, NSTEPS, **args))
    assert [n for n, a in fwd] == [forward] * NSTEPS and all(a['nsteps'] == 1 for n, a in fwd)
    assert len(bwd) == 1
    check_call(bwd[0], name, NSTEPS, null, **numbers)
    assert w.grad is not None and bool(torch.isfinite(w.grad).all())
    if operator == 'grad':
        assert args['operator'].grad is not None


def test_advance_and_evolve_make_the_same_calls_on_a_forced_solver(gpu_device):
    s = solver(force=True, drag=DRAG)
    names = []
    for entry in (s.advance, s.evolve):
        fwd, bwd = backward_calls(s, lambda: entry(field(4, grad=True), NSTEPS))
        names.append(([n for n, a in fwd], [n for n, a in bwd]))
    assert names[0] == names[1] == (['nns_spec_ns_step_forced_f32'] * NSTEPS, ['nns_spec_ns_step_adjoint_f32'])
    s = solver(buoyancy=BUOY, **SCALAR)
    names = []
    for entry in (lambda w, t: s.advance_scalar(w, t, NSTEPS), lambda w, t: s.evolve(w, NSTEPS, theta=t)):
        fwd, bwd = backward_calls(s, lambda: entry(field(4, grad=True), field(5, grad=True)))
        names.append(([n for n, a in fwd], [n for n, a in bwd]))
    assert names[0] == names[1] == (['nns_spec_ns_step_buoyant_f32'] * NSTEPS, ['nns_spec_ns_step_scalar_adjoint_f32'])
