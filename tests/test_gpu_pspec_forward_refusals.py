"""What the forward-mode methods of nns.periodic.PeriodicSolver refuse, and how their four steps agree (step_tangent, step_tangent_scalar,
step_tangents, step_tangents_scalar, lyapunov_exponent(_scalar), lyapunov_spectrum(_scalar), tangent_gram(_scalar)): for a call wrong in one
argument the exception's type and a message that names the method and the argument, before any launch; and the step of K = 1 members bit for
bit the step of one tangent.  64x64 with B = 2, the smallest the solver takes.  That the base of all four is bitwise ``step``'s and that
without buoyancy dwhat is bitwise ``step_tangent``'s is asserted in test_gpu_pspec_tangent.py, test_gpu_pspec_scalar_tangent.py,
test_gpu_pspec_lyapunov.py and test_gpu_pspec_scalar_lyapunov.py."""
import numpy as np
import pytest
import torch

import pspec_scalar_tangent_cases as TC

pytestmark = pytest.mark.gpu

C = (64, 64, 2) + tuple(TC.CASES[0][3:])
K = 3
FLOW = ('step_tangent', 'lyapunov_exponent', 'step_tangents', 'lyapunov_spectrum', 'tangent_gram')
SCALAR = tuple(m + '_scalar' for m in FLOW)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device='cuda')


class Setup(object):
    """A plain solver and one with kappa, a state of each kind and good tangents of every layout; built once, never stepped."""

    def __init__(self):
        from nns.periodic import PeriodicSolver
        d = TC.inputs(C)
        self.plain = PeriodicSolver(C[0], C[1], d['dt'], TC.RHO, TC.NU, drag=TC.DRAG)
        self.solver = TC.solver('buoyant', C, d['dt'])
        u0, v0, theta0 = dev(d['u0']), dev(d['v0']), dev(d['theta0'])
        self.plain_state = self.plain.init(u0, v0)
        self.free, self.state = self.solver.init(u0, v0), self.solver.init(u0, v0, theta0)
        dw = np.stack([np.roll(d['dw'], k, axis=1) for k in range(K)])
        dth = np.stack([np.roll(d['dtheta'], k, axis=2) for k in range(K)])
        self.many = self.solver.init_tangents_scalar(dev(dw), dev(dth))           # (dwhat, dthat) [K, B, my1, nx, 2]
        self.one = tuple(t[0].clone() for t in self.many)                         # (dwhat, dthat) [B, my1, nx, 2]

    def call(self, method, solver=None, state=None, dwhat=None, dthat=None, nsteps=2, every=1, weight=1.0):
        """The call of ``method`` with good arguments but those given."""
        scalar, many = method.endswith('_scalar'), 'tangents' in method or 'spectrum' in method or 'gram' in method
        solver = (self.solver if solver is None else solver)
        good = self.many if many else self.one
        spectra = (good[0] if dwhat is None else dwhat[0],) + ((good[1] if dthat is None else dthat[0],) if scalar else ())
        f = getattr(solver, method)
        if 'gram' in method:
            return f(*spectra, *((weight,) if scalar else ()))
        state = (self.state if scalar else self.free) if state is None else state
        if 'lyapunov' in method:
            return f(state, *spectra, nsteps, every, *((weight,) if scalar else ()))
        return f(state, *spectra, nsteps)


@pytest.fixture(scope='module')
def S(gpu_device):
    return Setup()


def refused(S, exc, method, words, **kw):
    """The call raises exc, and its message holds every one of ``words``."""
    with pytest.raises(exc) as e:
        S.call(method, **kw)
    msg = str(e.value)
    print('%s(%s): %s: %s' % (method, ', '.join(kw), type(e.value).__name__, msg))
    assert type(e.value) is exc, (method, kw, type(e.value))
    for w in words:
        assert w in msg, (method, kw, w, msg)


def bad_spectra(good, many):
    """(what is wrong, the tensor or non-tensor, exception) for a spectrum argument whose good value is ``good``."""
    shape = tuple(good.shape)
    out = [('a non-tensor', None, TypeError), ('a list', [0.0], TypeError), ('float64', good.double(), ValueError),
           ('trailing shape', torch.zeros(shape[:-2] + (shape[-2] - 1, 2), device='cuda'), ValueError),
           ('rank', good[0], ValueError),
           ('strides', good.transpose(-3, -2).contiguous().transpose(-3, -2), ValueError)]
    assert not out[-1][1].is_contiguous() and tuple(out[-1][1].shape) == shape
    return out


@pytest.mark.parametrize('method', FLOW + SCALAR)
def test_a_wrong_spectrum_is_refused_by_name(S, method):
    scalar, many = method.endswith('_scalar'), 'tangents' in method or 'spectrum' in method or 'gram' in method
    good = S.many if many else S.one
    for i, name in enumerate(('dwhat', 'dthat') if scalar else ('dwhat',)):
        for what, bad, exc in bad_spectra(good[i], many):
            refused(S, exc, method, (method, name), **{name: (bad,)})
        if 'gram' not in method:                                       # a Gram matrix has no state to tell the batch from
            batch = good[i][..., :1, :, :, :].contiguous()
            refused(S, ValueError, method, (method, name), **{name: (batch,)})
    if scalar:                                                         # dthat of another shape than dwhat
        other = good[1][:1].contiguous()
        refused(S, ValueError, method, (method, 'dthat'), dthat=(other,))


@pytest.mark.parametrize('method', [m for m in FLOW + SCALAR if 'tangents' in m or 'spectrum' in m or 'gram' in m])
@pytest.mark.parametrize('count', [0, 33])
def test_K_out_of_range_is_refused(S, method, count):
    wide = torch.zeros((count,) + tuple(S.many[0].shape[1:]), device='cuda')
    refused(S, ValueError, method, (method, 'K = %d' % count, '[1, 32]'), dwhat=(wide,), dthat=(wide.clone(),))


@pytest.mark.parametrize('method', [m for m in FLOW if 'gram' not in m])
def test_a_state_with_a_scalar_is_refused_by_a_flow_method(S, method):
    refused(S, NotImplementedError, method, (method, 'tangent of the scalar system is not built', '_scalar'), state=S.state)


@pytest.mark.parametrize('method', [m for m in SCALAR if 'gram' not in m])
def test_a_state_without_a_scalar_is_refused_by_a_scalar_method(S, method):
    refused(S, ValueError, method, (method, 'carries no scalar', method.replace('_scalar', '')), state=S.free)


@pytest.mark.parametrize('method', SCALAR)
def test_a_solver_without_kappa_is_refused_by_a_scalar_method(S, method):
    refused(S, ValueError, method, (method, 'kappa'), solver=S.plain, state=S.plain_state)


@pytest.mark.parametrize('method', [m for m in FLOW + SCALAR if 'gram' not in m])
def test_wrong_counts_are_refused(S, method):
    refused(S, ValueError, method, ('nsteps', '-1'), nsteps=-1)
    refused(S, TypeError, method, ('nsteps',), nsteps=1.0)
    if 'lyapunov' in method:
        refused(S, ValueError, method, ('renormalize_every', '>= 1'), every=0)
        refused(S, ValueError, method, ('nsteps', '>= 1'), nsteps=0)


@pytest.mark.parametrize('method', [m for m in SCALAR if 'lyapunov' in m or 'gram' in m])
def test_a_wrong_scalar_weight_is_refused(S, method):
    for w in (0.0, -1.0, float('nan')):
        refused(S, ValueError, method, ('scalar_weight',), weight=w)
    refused(S, TypeError, method, ('scalar_weight',), weight='1')


def test_nothing_was_launched(S):
    """Last in the file: no refusal above stepped a state, grew a workspace or touched a tangent."""
    fresh = Setup()
    for st, ref in ((S.plain_state, fresh.plain_state), (S.free, fresh.free), (S.state, fresh.state)):
        assert st.steps == 0 and st.clock is None and torch.equal(st.what, ref.what) and st.work.numel() == ref.work.numel()
    assert torch.equal(S.state.that, fresh.state.that)
    for a, b in zip(S.many + S.one, fresh.many + fresh.one):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------- K = 1 is the single tangent
def agreement_solver(kind):
    """'forced': the steady per-grid force and drag, a passive scalar; 'buoyant-linear-stochastic': also buoyancy, the linear table and noise."""
    d = TC.inputs(C)
    if kind == 'forced':
        s = TC.solver('passive', C, d['dt'])
    else:
        s = TC.solver('buoyant-linear', C, d['dt'])
        s.ring_forcing(*TC.LAC.ring(C), seed=TC.SEED)
    s.set_forcing(dev(d['fx']), dev(d['fy']))
    return s, d


@pytest.mark.parametrize('kind', ['forced', 'buoyant-linear-stochastic'])
def test_one_member_is_bitwise_the_single_tangent(gpu_device, kind):
    s, d = agreement_solver(kind)
    u0, v0 = dev(d['u0']), dev(d['v0'])
    dwhat, dthat = s.init_tangents_scalar(dev(d['dw'][None]), dev(d['dtheta'][None]))
    assert tuple(dwhat.shape) == (1, 2, s.my1, 64, 2)
    # the flow alone: a state without a scalar
    one, many = s.init(u0, v0), s.init(u0, v0)
    d1, dk = dwhat[0].clone(), dwhat.clone()
    s.step_tangent(one, d1, 2)
    s.step_tangents(many, dk, 2)
    assert torch.equal(dk[0], d1) and not torch.equal(d1, dwhat[0]) and torch.equal(one.what, many.what)
    assert one.steps == many.steps == 2 and (one.clock is None or (torch.equal(one.clock, many.clock) and int(one.clock) == 2))
    # the flow and its scalar
    theta0 = dev(d['theta0'])
    one, many = s.init(u0, v0, theta0), s.init(u0, v0, theta0)
    d1, t1, dk, tk = dwhat[0].clone(), dthat[0].clone(), dwhat.clone(), dthat.clone()
    s.step_tangent_scalar(one, d1, t1, 2)
    s.step_tangents_scalar(many, dk, tk, 2)
    assert torch.equal(dk[0], d1) and torch.equal(tk[0], t1) and not torch.equal(d1, dwhat[0]) and not torch.equal(t1, dthat[0])
    assert torch.equal(one.what, many.what) and torch.equal(one.that, many.that)
    assert one.steps == many.steps == 2 and (one.clock is None or (torch.equal(one.clock, many.clock) and int(one.clock) == 2))
