"""Thin, typed wrappers over the C ABI (include/nns.h) for torch device tensors.

PyTorch is plumbing here (device memory + the current HIP stream); all arithmetic happens in the
hand-written HIP kernels of csrc/.  Every function takes contiguous CUDA(HIP) tensors shaped
[nx, ny] or [batch, nx, ny] in float32 or float64, enqueues ONE stream-ordered call on
torch's current stream and returns its outputs as tensors.  Errors raise nns._lib.NnsError with
the library's message; there is no CPU fallback.
"""
import ctypes
import numbers

import torch

from . import _lib
from ._lib import BcList, check

KIND = {'dirichlet': 0, 'neumann': 1}
SIDE = {'left': 0, 'right': 1, 'bottom': 2, 'top': 3}


def _prec(precise):
    """The C ABI's `precise` argument: 0 = all-float32 transforms (on differenced lines); 1 / True = the library picks -- all-float32 while
    the viscous amplification nu pi N / (sqrt(3) L) <= 8, else float64 forward transforms; 2 = float64 forward transforms always."""
    return 2 if (precise is not True and precise is not False and int(precise) >= 2) else int(bool(precise))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _suffix(t):
    if t.dtype == torch.float32:
        return '_f32'
    if t.dtype == torch.float64:
        return '_f64'
    raise TypeError("fields must be float32 or float64, got %s" % t.dtype)


def _dims(t):
    if t.dim() == 2:
        return 1, t.shape[0], t.shape[1]
    if t.dim() == 3:
        return t.shape[0], t.shape[1], t.shape[2]
    raise ValueError("field must be [nx, ny] or [batch, nx, ny], got shape %s" % (tuple(t.shape),))


def _chk(*ts):
    t0 = ts[0]
    for t in ts:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise TypeError("expected a CUDA/HIP torch tensor (the HIP path has no CPU fallback)")
        if not t.is_contiguous():
            raise ValueError("fields must be C-contiguous")
        if t.dtype != t0.dtype or t.shape != t0.shape or t.device != t0.device:
            raise ValueError("all fields of one call must share dtype, shape and device")
    return _suffix(t0), _dims(t0)


def make_bc_list(bcs):
    """bcs: iterable of objects with .type/.boundary/.value/.dx/.dy (nns.boundary classes or the
    reference's own) or of (kind, side, value, dx, dy) tuples."""
    out = BcList()
    bcs = list(bcs)
    if len(bcs) > _lib.NNS_MAX_BC:
        raise ValueError("at most %d boundary conditions per list" % _lib.NNS_MAX_BC)
    out.n = len(bcs)
    for i, b in enumerate(bcs):
        if isinstance(b, (tuple, list)):
            kind, side, value, dx, dy = b
        else:
            kind, side, value, dx, dy = b.type, b.boundary, b.value, b.dx, b.dy
        out.kind[i], out.side[i] = KIND[kind], SIDE[side]
        out.value[i], out.dx[i], out.dy[i] = float(value), float(dx), float(dy)
    return out


def _call(name, suf, *args):
    check(getattr(_lib.lib(), name + suf)(*args), name + suf)


def _p(t):
    return t.data_ptr()


def _query_bytes(name, *args):
    """The size a workspace query returns through its trailing size_t* argument."""
    n = ctypes.c_size_t(0)
    check(getattr(_lib.lib(), name)(*args, ctypes.byref(n)), name)
    return n.value


def _workspace(nbytes, like):
    """nbytes of scratch as elements of like's dtype, on its device."""
    return torch.empty(nbytes // like.element_size(), dtype=like.dtype, device=like.device)


def _halo_msgs(who, halo_top, halo_bot, u, B, ny, halo_grid0=None):
    """The two [3, Bh, ny] halo messages of a row slab of B grids; returns Bh.  halo_grid0 None: Bh = B; otherwise the messages may cover a larger
    batch, of which the call takes grids halo_grid0 .. halo_grid0 + B - 1."""
    exact = halo_grid0 is None
    g0 = 0 if exact else halo_grid0
    Bh = halo_top.shape[1] if halo_top.dim() == 3 else -1
    for h in (halo_top, halo_bot):
        if not (h.is_cuda and h.is_contiguous() and h.dtype == u.dtype and tuple(h.shape) == (3, Bh, ny) and 0 <= g0 and g0 + B <= Bh
                and (Bh == B or not exact)):
            raise ValueError("%s: halo messages must be contiguous [3, %s%d, %d] %s" % (
                who, '' if exact else '>= ', g0 + B, ny, "device tensors of the fields' dtype" if exact else "float32 device tensors"))
    return Bh


# ----------------------------------------------------------------------------- boundary
def bc_apply_(A, bcs):
    suf, (B, nx, ny) = _chk(A)
    bl = bcs if isinstance(bcs, BcList) else make_bc_list(bcs)
    _call('nns_bc_apply', suf, _p(A), B, nx, ny, bl, _stream())
    return A


# ----------------------------------------------------------------------------- chorin_fd
def fd_predictor_explicit(un, vn, un1, vn1, dt, dx, dy, nu):
    suf, (B, nx, ny) = _chk(un, vn, un1, vn1)
    ui, vi = torch.empty_like(un), torch.empty_like(vn)
    _call('nns_fd_predictor_explicit', suf, _p(un), _p(vn), _p(un1), _p(vn1), _p(ui), _p(vi), B, nx, ny,
          dt, dx, dy, nu, _stream())
    return ui, vi


def fd_predictor_explicit_corrected(un, vn, un1, vn1, dt, dx, dy, nu):
    """The explicit predictor with the true y-advection (an option of the build, not reference behaviour)."""
    suf, (B, nx, ny) = _chk(un, vn, un1, vn1)
    ui, vi = torch.empty_like(un), torch.empty_like(vn)
    _call('nns_fd_predictor_explicit_corrected', suf, _p(un), _p(vn), _p(un1), _p(vn1), _p(ui), _p(vi), B, nx, ny,
          dt, dx, dy, nu, _stream())
    return ui, vi


def fd_predictor_adi(un, vn, un1, vn1, dt, dx, dy, nu, corrected=False, column_slab=False):
    """corrected=True: the second ADI solve runs along axis 1 (an option of the build; nx != ny allowed).
    column_slab=True: the inputs are a column slab [nx, nyl] of a square grid (nns.slab.SlabChorinFD)."""
    if corrected and column_slab:
        raise ValueError("fd_predictor_adi: column slabs are for the reference ADI (both solves along axis 0)")
    suf, (B, nx, ny) = _chk(un, vn, un1, vn1)
    ui, vi = torch.empty_like(un), torch.empty_like(vn)
    work = _workspace(_lib.lib().nns_fd_predictor_adi_workspace(B, nx, ny, un.element_size()), un)
    _call('nns_fd_predictor_adi_corrected' if corrected else 'nns_fd_predictor_adi_colslab' if column_slab else 'nns_fd_predictor_adi', suf, _p(un), _p(vn), _p(un1), _p(vn1), _p(ui), _p(vi), _p(work), B, nx, ny,
          dt, dx, dy, nu, _stream())
    return ui, vi


def fd_pressure_rhs(ui, vi, dt, dx, dy, rho):
    suf, (B, nx, ny) = _chk(ui, vi)
    C = torch.empty_like(ui)
    _call('nns_fd_pressure_rhs', suf, _p(ui), _p(vi), _p(C), B, nx, ny, dt, dx, dy, rho, _stream())
    return C


def _sor_hint(hint, B, p):
    if hint is None:
        return None
    if not (isinstance(hint, torch.Tensor) and hint.is_cuda and hint.dtype == p.dtype and hint.is_contiguous() and tuple(hint.shape) == (B, 2)):
        raise ValueError("SOR hint: the info tensor [batch, 2] of a previous solve of the same grids (same dtype and device) expected")
    return _p(hint)


def fd_sor_(p, C, dx, dy, beta, tol, max_sweeps, hint=None):
    """In place on p.  Returns the device info tensor [batch, 2] = (sweeps done, last err).  hint: the info of the previous solve of the same
    grids in a time loop (sizes the first speculative batch of sweeps; the result does not depend on it)."""
    suf, (B, nx, ny) = _chk(p, C)
    info = torch.empty(B, 2, dtype=p.dtype, device=p.device)
    work = _workspace(_lib.lib().nns_fd_sor_workspace(B, nx, ny, p.element_size()), p)
    _call('nns_fd_sor_hint', suf, _p(p), _p(C), _p(info), _sor_hint(hint, B, p), _p(work), B, nx, ny, dx, dy, beta, tol, int(max_sweeps), _stream())
    return info


def fd_sor_redblack_(p, C, dx, dy, beta, tol, max_sweeps):
    """Red-black SOR, in place on p (an option of the build).  Returns the device info tensor [batch, 2]."""
    suf, (B, nx, ny) = _chk(p, C)
    info = torch.empty(B, 2, dtype=p.dtype, device=p.device)
    nbytes = _lib.lib().nns_fd_sor_redblack_workspace(B, nx, ny, p.element_size(), int(max_sweeps))     # 0: the grids fit LDS
    work = _workspace(nbytes, p) if nbytes else None
    _call('nns_fd_sor_redblack', suf, _p(p), _p(C), _p(info), _p(work) if nbytes else None, B, nx, ny, dx, dy, beta, tol,
          int(max_sweeps), _stream())
    return info


MG_FIRST_CHUNK = 4        # cycles enqueued before the first status read when no hint is given
MG_CHUNK = 2              # cycles per later chunk (the f64 solves of a time loop need 5-7 cycles at tol 1e-6)


def fd_poisson_mg_workspace(B, nx, ny, elem_size):
    return _query_bytes('nns_fd_poisson_mg_workspace', int(B), int(nx), int(ny), int(elem_size))


def fd_poisson_mg_(p, C, dx, dy, tol=1e-6, max_cycles=30, hint=None):
    """Multigrid solve of the pressure equation (nns_fd_poisson_mg_*), in place on p.  Returns the device info tensor [batch, 2] = (cycles done,
    max|r_k| / max|r_0|), the layout of fd_sor_'s.  Cycles are enqueued in chunks; after each chunk ONE host sync reads the grids' active flags,
    and the solve goes on while any grid is active (each grid stops on its own, on the device) and fewer than max_cycles have run.  hint: the
    info of the previous solve of the same grids (a time loop) sizes the first chunk; the result does not depend on it."""
    suf, (B, nx, ny) = _chk(p, C)
    max_cycles = int(max_cycles)
    if max_cycles < 0:
        raise ValueError("fd_poisson_mg_: max_cycles must be >= 0")
    info = torch.empty(B, 2, dtype=p.dtype, device=p.device)
    nbytes = fd_poisson_mg_workspace(B, nx, ny, p.element_size())
    work = torch.empty(nbytes, dtype=torch.uint8, device=p.device)
    first = MG_FIRST_CHUNK
    if hint is not None:
        _sor_hint(hint, B, p)
        first = max(1, int(hint[:, 0].max().item()))
    done, chunk, resume = 0, min(first, max_cycles), 0
    active = work[:4 * B].view(torch.int32)
    while True:
        _call('nns_fd_poisson_mg', suf, _p(p), _p(C), _p(info), _p(work), B, nx, ny, float(dx), float(dy), float(tol), chunk, resume, _stream())
        done += chunk
        resume = 1
        if done >= max_cycles or not bool(active.any().item()):
            return info
        chunk = min(MG_CHUNK, max_cycles - done)


def fd_sor_redblack_halfsweep_(p, C, err, gi0, colour, dx, dy, beta):
    """One red-black half-sweep in place on a row slab p [nxl, ny] (rows 0 and nxl-1 = halo / boundary rows).
    err: a zeroed one-element tensor of p's dtype; afterwards err.max-accumulates max|p_new - p_old| (bit pattern)."""
    if p.dim() != 2 or p.shape != C.shape or not p.is_cuda or not p.is_contiguous() or not C.is_contiguous():
        raise ValueError("fd_sor_redblack_halfsweep_: p, C must be contiguous 2-D device tensors of one shape")
    _call('nns_fd_sor_redblack_halfsweep', _suffix(p), _p(p), _p(C), _p(err), p.shape[0], p.shape[1], int(gi0), int(colour), dx, dy, beta, _stream())
    return err


def fd_sor_redblack_halfsweep_gated_(p, C, err, prev_err, tol, gi0, colour, dx, dy, beta):
    """The half-sweep as one link of a pre-enqueued chain (nns_fd_sor_redblack_halfsweep_gated_*): it runs only if the
    one-element device tensor prev_err (the previous sweep's error, already max-reduced over the ranks) is > tol."""
    if p.dim() != 2 or p.shape != C.shape or not p.is_cuda or not p.is_contiguous() or not C.is_contiguous():
        raise ValueError("fd_sor_redblack_halfsweep_gated_: p, C must be contiguous 2-D device tensors of one shape")
    _call('nns_fd_sor_redblack_halfsweep_gated', _suffix(p), _p(p), _p(C), _p(err), _p(prev_err), float(tol), p.shape[0], p.shape[1], int(gi0), int(colour),
          dx, dy, beta, _stream())
    return err


def fd_correction(ui, vi, p, dt, dx, dy):
    suf, (B, nx, ny) = _chk(ui, vi, p)
    u, v = torch.empty_like(ui), torch.empty_like(vi)
    _call('nns_fd_correction', suf, _p(ui), _p(vi), _p(p), _p(u), _p(v), B, nx, ny, dt, dx, dy, _stream())
    return u, v


def fd_step_explicit_fits(nx, ny, dtype):
    """Does the one-launch explicit step apply to this grid (p and its right-hand side in one workgroup's LDS)?"""
    return bool(_lib.lib().nns_fd_step_explicit_fits(int(nx), int(ny), 8 if dtype == torch.float64 else 4))


def fd_step_explicit(un, vn, un1, vn1, p, u_bcl, v_bcl, p_bcl, dt, dx, dy, rho, nu, beta, tol, max_sweeps, corrected=False, out=None, p_copy=None, hint=None):
    """chorin_fd's explicit step in ONE launch (nns_fd_step_explicit_*): predictor, boundary lists, pressure solve, correction.  p is updated in
    place (and copied to p_copy when given); returns (u, v, info) with u, v = `out` (two fields that are not inputs) or new tensors."""
    suf, (B, nx, ny) = _chk(un, vn, un1, vn1, p)
    u, v = out if out is not None else (torch.empty_like(un), torch.empty_like(un))
    _chk(un, u, v)
    if p_copy is not None:
        _chk(un, p_copy)
    info = torch.empty(B, 2, dtype=p.dtype, device=p.device)
    work = _workspace(_lib.lib().nns_fd_sor_workspace(B, nx, ny, p.element_size()), p)
    _call('nns_fd_step_explicit', suf, _p(un), _p(vn), _p(un1), _p(vn1), _p(p), u_bcl, v_bcl, p_bcl, _p(u), _p(v), _p(p_copy) if p_copy is not None else None,
          _p(info), _sor_hint(hint, B, p), _p(work), B, nx, ny, dt, dx, dy, rho, nu, beta, tol, int(max_sweeps), int(bool(corrected)), _stream())
    return u, v, info


def coarsen(u, v, p, agg_x, agg_y, jfill=None):
    """Block means of the [T, nx, ny] device sequences u, v, p over agg_x x agg_y cells (nns_coarsen_*).
    jfill: coarse columns filled per row (the rest are 0); default ny / agg_y."""
    if not (u.dim() == 3 and u.shape == v.shape == p.shape and u.dtype == v.dtype == p.dtype and u.is_cuda and v.is_cuda and p.is_cuda):
        raise ValueError("coarsen: u, v, p must be device tensors of one [T, nx, ny] shape and dtype")
    if u.dtype not in (torch.float32, torch.float64):
        raise TypeError("coarsen: float32 or float64 fields")
    if not (u.is_contiguous() and v.is_contiguous() and p.is_contiguous()):
        raise ValueError("coarsen: contiguous tensors required")
    T, nx, ny = u.shape
    if agg_x < 1 or agg_y < 1 or nx % agg_x or ny % agg_y:
        raise ValueError("coarsen: nx=%d, ny=%d must be multiples of agg_x=%d, agg_y=%d" % (nx, ny, agg_x, agg_y))
    out = [torch.empty(T, nx // agg_x, ny // agg_y, dtype=u.dtype, device=u.device) for _ in range(3)]
    _call('nns_coarsen', _suffix(u), _p(u), _p(v), _p(p), _p(out[0]), _p(out[1]), _p(out[2]), T, nx, ny, int(agg_x), int(agg_y),
          ny // agg_y if jfill is None else int(jfill), _stream())
    return tuple(out)


# ----------------------------------------------------------------------------- direct_fd
def fd_build_b(u, v, dt, dx, dy, rho):
    suf, (B, nx, ny) = _chk(u, v)
    b = torch.empty_like(u)
    _call('nns_fd_build_b', suf, _p(u), _p(v), _p(b), B, nx, ny, dt, dx, dy, rho, _stream())
    return b


def fd_jacobi_(p, b, dx, dy, nit, p_bc):
    suf, (B, nx, ny) = _chk(p, b)
    bl = p_bc if isinstance(p_bc, BcList) else make_bc_list(p_bc)
    tmp = torch.empty_like(p)
    _call('nns_fd_jacobi', suf, _p(p), _p(tmp), _p(b), B, nx, ny, dx, dy, int(nit), bl, _stream())
    return p


def fd_direct_update(un, vn, p, dt, dx, dy, rho, nu):
    suf, (B, nx, ny) = _chk(un, vn, p)
    u, v = torch.empty_like(un), torch.empty_like(vn)
    _call('nns_fd_direct_update', suf, _p(un), _p(vn), _p(p), _p(u), _p(v), B, nx, ny, dt, dx, dy, rho, nu, _stream())
    return u, v


# ----------------------------------------------------------------------------- periodic residual
def fd_residual(u, v, p, u_prev, v_prev, dt, dx, dy, rho, nu, stencil=5, out=None):
    suf, (B, nx, ny) = _chk(u, v, p, u_prev, v_prev)
    ru, rv, rd = out if out is not None else (torch.empty_like(u), torch.empty_like(u), torch.empty_like(u))
    _call('nns_fd_residual', suf, _p(u), _p(v), _p(p), _p(u_prev), _p(v_prev), _p(ru), _p(rv), _p(rd), B, nx, ny,
          dt, dx, dy, rho, nu, int(stencil), _stream())
    return ru, rv, rd


def fd_residual_halo(u, v, p, u_prev, v_prev, halo_top, halo_bot, dt, dx, dy, rho, nu, stencil=5, rows=None, out=None):
    """fd_residual on local rows `rows` = (begin, end) of a row slab [B, nloc, ny] whose rows -1 / nloc are the
    [3, B, ny] messages halo_top / halo_bot (nns_fd_residual_halo_*)."""
    suf, (B, nx, ny) = _chk(u, v, p, u_prev, v_prev)
    _halo_msgs('fd_residual_halo', halo_top, halo_bot, u, B, ny)
    ru, rv, rd = out if out is not None else (torch.empty_like(u), torch.empty_like(u), torch.empty_like(u))
    r0, r1 = rows if rows is not None else (0, nx)
    _call('nns_fd_residual_halo', suf, _p(u), _p(v), _p(p), _p(u_prev), _p(v_prev), _p(halo_top), _p(halo_bot), _p(ru), _p(rv), _p(rd),
          B, nx, ny, int(r0), int(r1), dt, dx, dy, rho, nu, int(stencil), _stream())
    return ru, rv, rd


def fd_residual_bwd(u, v, g_u, g_v, g_div, dt, dx, dy, rho, nu, stencil=5, want_prev=True):
    """Vector-Jacobian product of fd_residual: returns (grad_u, grad_v, grad_p, grad_u_prev, grad_v_prev)
    (the last two None unless want_prev)."""
    suf, (B, nx, ny) = _chk(u, v, g_u, g_v, g_div)
    gu, gv, gp = torch.empty_like(u), torch.empty_like(u), torch.empty_like(u)
    gup, gvp = (torch.empty_like(u), torch.empty_like(u)) if want_prev else (None, None)
    _call('nns_fd_residual_bwd', suf, _p(u), _p(v), _p(g_u), _p(g_v), _p(g_div), _p(gu), _p(gv), _p(gp),
          _p(gup) if want_prev else None, _p(gvp) if want_prev else None, B, nx, ny, dt, dx, dy, rho, nu, int(stencil), _stream())
    return gu, gv, gp, gup, gvp


class FdResidualFn(torch.autograd.Function):
    """fd_residual as an autograd node (forward: nns_fd_residual, backward: nns_fd_residual_bwd, the adjoint stencils)."""

    @staticmethod
    def forward(ctx, u, v, p, u_prev, v_prev, dt, dx, dy, rho, nu, stencil):
        u, v, p, u_prev, v_prev = (t.contiguous() for t in (u, v, p, u_prev, v_prev))
        ctx.save_for_backward(u, v)
        ctx.consts = (dt, dx, dy, rho, nu, stencil)
        return fd_residual(u, v, p, u_prev, v_prev, dt, dx, dy, rho, nu, stencil)

    @staticmethod
    def backward(ctx, g_u, g_v, g_d):
        u, v = ctx.saved_tensors
        dt, dx, dy, rho, nu, stencil = ctx.consts
        zero = lambda g: torch.zeros_like(u) if g is None else g.contiguous()
        want_prev = ctx.needs_input_grad[3] or ctx.needs_input_grad[4]
        gu, gv, gp, gup, gvp = fd_residual_bwd(u, v, zero(g_u), zero(g_v), zero(g_d), dt, dx, dy, rho, nu, stencil, want_prev)
        return (gu, gv, gp, gup, gvp) + (None,) * 6


def spec_residual(u, v, p, u_prev, v_prev, dt, Lx, Ly, rho, nu, precise=True, out=None):
    suf, (B, nx, ny) = _chk(u, v, p, u_prev, v_prev)
    if suf != '_f32':
        raise TypeError("spec_residual: float32 fields (the forward transforms run in float64 internally)")
    ru, rv, rd = out if out is not None else (torch.empty_like(u), torch.empty_like(u), torch.empty_like(u))
    check(_lib.lib().nns_spec_residual_f32(_p(u), _p(v), _p(p), _p(u_prev), _p(v_prev), _p(ru), _p(rv), _p(rd), B, nx, ny,
                                           dt, Lx, Ly, rho, nu, _prec(precise), _stream()), 'nns_spec_residual_f32')
    return ru, rv, rd


def residual_both(u, v, p, u_prev, v_prev, dt, Lx, Ly, rho, nu, precise=True, out_fd=None, out_spec=None, rowpass_only=False):
    """FD 5-point AND spectral residual of the same inputs (the 'stencil + spectral residual' of BASELINE.json) by
    nns_residual_both_f32: spectral column pass, then ONE row pass that also evaluates the stencil.
    Returns ((fd r_u, r_v, r_div), (spectral r_u, r_v, r_div)).  rowpass_only: out_spec already holds the column pass's
    partials (spec_residual_xpass) and only the second launch runs."""
    suf, (B, nx, ny) = _chk(u, v, p, u_prev, v_prev)
    if suf != '_f32':
        raise TypeError("residual_both: float32 fields")
    fo = out_fd if out_fd is not None else tuple(torch.empty_like(u) for _ in range(3))
    so = out_spec if out_spec is not None else tuple(torch.empty_like(u) for _ in range(3))
    fn = _lib.lib().nns_residual_both_rowpass_f32 if rowpass_only else _lib.lib().nns_residual_both_f32
    check(fn(_p(u), _p(v), _p(p), _p(u_prev), _p(v_prev), _p(fo[0]), _p(fo[1]), _p(fo[2]), _p(so[0]), _p(so[1]), _p(so[2]), B, nx, ny,
             dt, Lx, Ly, rho, nu, _prec(precise), _stream()), 'nns_residual_both_f32')
    return fo, so


def spec_residual_xpass(u, v, p, Lx, rho, nu, precise=True, out=None):
    suf, (B, nx, ny) = _chk(u, v, p)
    if suf != '_f32':
        raise TypeError("spec_residual_xpass: float32 fields")
    ru, rv, rd = out if out is not None else (torch.empty_like(u), torch.empty_like(u), torch.empty_like(u))
    check(_lib.lib().nns_spec_residual_xpass_f32(_p(u), _p(v), _p(p), _p(ru), _p(rv), _p(rd), B, nx, ny, Lx, rho, nu,
                                                 _prec(precise), _stream()), 'nns_spec_residual_xpass_f32')
    return ru, rv, rd


def spec_residual_xpass_seg(recv, send, B, nx, nyl, seg_rows, Lx, rho, nu, precise=True):
    """The column pass on the RECEIVE buffer of the slab all-to-all, recv [P, 3, B, seg_rows, nyl] (u, v, p from every source
    rank), writing its three partials into `send` of the same layout (the send buffer of the return all-to-all):
    nns_spec_residual_xpass_seg_f32."""
    _f32(recv, send)
    if recv.shape != send.shape or recv.dim() != 5 or recv.shape[1] != 3 or recv.shape[0] * seg_rows != nx or tuple(recv.shape[2:]) != (B, seg_rows, nyl):
        raise ValueError("spec_residual_xpass_seg: buffers must be [P, 3, %d, %d, %d] with P * seg_rows = nx = %d, got %s" % (B, seg_rows, nyl, nx, tuple(recv.shape)))
    fs = B * seg_rows * nyl                  # one field of one source rank
    e = recv.element_size()
    q = lambda t, f: t.data_ptr() + f * fs * e
    check(_lib.lib().nns_spec_residual_xpass_seg_f32(q(recv, 0), q(recv, 1), q(recv, 2), q(send, 0), q(send, 1), q(send, 2), B, nx, nyl,
                                                     int(seg_rows), 3 * fs, Lx, rho, nu, _prec(precise), _stream()), 'nns_spec_residual_xpass_seg_f32')
    return send


def residual_both_rowpass_halo(u, v, p, u_prev, v_prev, halo_top, halo_bot, sp_partials, dt, dx, Ly, rho, nu, precise=True, out_fd=None, halo_grid0=0):
    """The fused row pass on a row slab (nns_residual_both_rowpass_halo_f32): sp_partials holds the column pass's partials on
    entry and the spectral residual on return; returns ((fd r_u, r_v, r_div), sp_partials).  halo_top / halo_bot: [3, Bh, ny] messages;
    Bh may exceed this call's batch B -- the call then covers grids halo_grid0 .. halo_grid0 + B - 1 of the batch the messages were
    exchanged for (nns/slab.py: one halo exchange per step, batch chunks pipelined)."""
    suf, (B, nx, ny) = _chk(u, v, p, u_prev, v_prev, *sp_partials)
    if suf != '_f32':
        raise TypeError("residual_both_rowpass_halo: float32 fields")
    Bh = _halo_msgs('residual_both_rowpass_halo', halo_top, halo_bot, u, B, ny, halo_grid0)
    fo = out_fd if out_fd is not None else tuple(torch.empty_like(u) for _ in range(3))
    so = sp_partials
    off = halo_grid0 * ny * 4
    check(_lib.lib().nns_residual_both_rowpass_halo_f32(_p(u), _p(v), _p(p), _p(u_prev), _p(v_prev), _p(halo_top) + off, _p(halo_bot) + off,
                                                        _p(fo[0]), _p(fo[1]), _p(fo[2]), _p(so[0]), _p(so[1]), _p(so[2]), B, nx, ny, Bh * ny,
                                                        dt, dx, Ly, rho, nu, _prec(precise), _stream()), 'nns_residual_both_rowpass_halo_f32')
    return fo, so


def _seg_parts(got, B, nx, ny, what):
    """got [P, 3, B, nx, ny / P] (the receive buffer of the return all-to-all) -> (the three fields' pointers of source rank 0, seg_cols, seg_stride)."""
    _f32(got)
    P = got.shape[0] if got.dim() == 5 else 0
    if P < 1 or ny % P or tuple(got.shape) != (P, 3, B, nx, ny // P):
        raise ValueError("%s: partials must be [P, 3, %d, %d, ny / P] float32, got %s" % (what, B, nx, tuple(got.shape)))
    fs = B * nx * (ny // P)
    return [got.data_ptr() + f * fs * 4 for f in range(3)], ny // P, 3 * fs


def residual_both_rowpass_halo_seg(u, v, p, u_prev, v_prev, halo_top, halo_bot, got, dt, dx, Ly, rho, nu, precise=True, out_fd=None, out_spec=None, halo_grid0=0):
    """The fused row pass on a row slab with its column-pass partials read IN PLACE from `got` [P, 3, B, nloc, ny / P], the receive buffer
    of the slab step's return all-to-all (nns_residual_both_rowpass_halo_seg_f32): no scatter copy in between.  Returns
    ((fd r_u, r_v, r_div), (spectral r_u, r_v, r_div)), both as row slabs.  halo_top / halo_bot / halo_grid0 as residual_both_rowpass_halo."""
    suf, (B, nx, ny) = _chk(u, v, p, u_prev, v_prev)
    if suf != '_f32':
        raise TypeError("residual_both_rowpass_halo_seg: float32 fields")
    Bh = _halo_msgs('residual_both_rowpass_halo_seg', halo_top, halo_bot, u, B, ny, halo_grid0)
    parts, seg_cols, seg_stride = _seg_parts(got, B, nx, ny, 'residual_both_rowpass_halo_seg')
    fo = out_fd if out_fd is not None else tuple(torch.empty_like(u) for _ in range(3))
    so = out_spec if out_spec is not None else tuple(torch.empty_like(u) for _ in range(3))
    _chk(u, *fo, *so)
    off = halo_grid0 * ny * 4
    check(_lib.lib().nns_residual_both_rowpass_halo_seg_f32(_p(u), _p(v), _p(p), _p(u_prev), _p(v_prev), _p(halo_top) + off, _p(halo_bot) + off,
                                                            parts[0], parts[1], parts[2], seg_cols, seg_stride,
                                                            _p(fo[0]), _p(fo[1]), _p(fo[2]), _p(so[0]), _p(so[1]), _p(so[2]), B, nx, ny, Bh * ny,
                                                            dt, dx, Ly, rho, nu, _prec(precise), _stream()), 'nns_residual_both_rowpass_halo_seg_f32')
    return fo, so


def spec_residual_ypass_seg(u, v, p, u_prev, v_prev, got, dt, Ly, rho, nu, precise=True, out=None):
    """The spectral row pass with its partials read in place from `got` [P, 3, B, nloc, ny / P] (nns_spec_residual_ypass_seg_f32)."""
    suf, (B, nx, ny) = _chk(u, v, p, u_prev, v_prev)
    if suf != '_f32':
        raise TypeError("spec_residual_ypass_seg: float32 fields")
    parts, seg_cols, seg_stride = _seg_parts(got, B, nx, ny, 'spec_residual_ypass_seg')
    ro = out if out is not None else tuple(torch.empty_like(u) for _ in range(3))
    _chk(u, *ro)
    check(_lib.lib().nns_spec_residual_ypass_seg_f32(_p(u), _p(v), _p(p), _p(u_prev), _p(v_prev), parts[0], parts[1], parts[2], seg_cols, seg_stride,
                                                     _p(ro[0]), _p(ro[1]), _p(ro[2]), B, nx, ny, dt, Ly, rho, nu, _prec(precise), _stream()),
          'nns_spec_residual_ypass_seg_f32')
    return ro


def spec_resolve_precise(precise, nu, nx, Lx, ny, Ly):
    """The arithmetic a `precise` request resolves to for a whole evaluation: 0 or 2 (nns_spec_resolve_precise: the library's one policy,
    NNS_SPEC_F64 included)."""
    return int(_lib.lib().nns_spec_resolve_precise(_prec(precise), float(nu), int(nx), float(Lx), int(ny), float(Ly)))


# ----------------------------------------------------------------------------- slab message packing (nns/slab.py)
def _ptr_array(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _slab_fields(fields, what):
    t0 = fields[0]
    if not 1 <= len(fields) <= 4:
        raise ValueError("%s: 1 to 4 fields per message" % what)
    for t in fields:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype == t0.dtype and t.shape == t0.shape):
            raise ValueError("%s: fields must be contiguous device tensors of one shape and dtype" % what)
    return _suffix(t0)


def slab_gather_lines(fields, msg, nouter, outer_stride, line_off, length, elem_stride=1):
    """msg[f, o, e] = fields[f].flat[o * outer_stride + line_off + e * elem_stride] (one launch, nns_slab_gather_lines_*)."""
    suf = _slab_fields(fields, 'slab_gather_lines')
    if not (msg.is_cuda and msg.is_contiguous() and msg.dtype == fields[0].dtype and msg.numel() == len(fields) * nouter * length):
        raise ValueError("slab_gather_lines: msg must hold nfields * nouter * len elements")
    if (nouter - 1) * outer_stride + line_off + (length - 1) * elem_stride >= fields[0].numel():
        raise ValueError("slab_gather_lines: line runs past the end of the field")
    _call('nns_slab_gather_lines', suf, _ptr_array(fields), len(fields), _p(msg), nouter, outer_stride, line_off, length, elem_stride, _stream())
    return msg


def slab_scatter_lines(msg, fields, nouter, outer_stride, line_off, length, elem_stride=1):
    """The reverse of slab_gather_lines: writes the message's lines into the fields (nns_slab_scatter_lines_*)."""
    suf = _slab_fields(fields, 'slab_scatter_lines')
    if not (msg.is_cuda and msg.is_contiguous() and msg.dtype == fields[0].dtype and msg.numel() == len(fields) * nouter * length):
        raise ValueError("slab_scatter_lines: msg must hold nfields * nouter * len elements")
    if (nouter - 1) * outer_stride + line_off + (length - 1) * elem_stride >= fields[0].numel():
        raise ValueError("slab_scatter_lines: line runs past the end of the field")
    _call('nns_slab_scatter_lines', suf, _p(msg), _ptr_array(fields), len(fields), nouter, outer_stride, line_off, length, elem_stride, _stream())
    return fields


def slab_transpose_pack(fields, send, P):
    """Row slabs fields[f] [B, nloc, ny] -> send [P, F, B, nloc, ny / P] (nns_slab_transpose_pack_*)."""
    suf = _slab_fields(fields, 'slab_transpose_pack')
    B, nloc, ny = fields[0].shape
    if not (send.is_cuda and send.is_contiguous() and send.dtype == fields[0].dtype and tuple(send.shape) == (P, len(fields), B, nloc, ny // P) and ny % P == 0):
        raise ValueError("slab_transpose_pack: send must be [%d, %d, %d, %d, %d]" % (P, len(fields), B, nloc, ny // P))
    _call('nns_slab_transpose_pack', suf, _ptr_array(fields), len(fields), _p(send), B, nloc, ny, P, _stream())
    return send


def slab_pack_halo(fields, send, first, last, g0, P):
    """transpose_pack of grids [g0, g0 + Bc) of the row slabs fields[f] [B, nloc, ny] into send [P, F, Bc, nloc, ny / P] and -- first / last not
    None -- the edge rows of ALL B grids into first / last [F, B, ny], in ONE launch (nns_slab_pack_halo_*)."""
    suf = _slab_fields(fields, 'slab_pack_halo')
    B, nloc, ny = fields[0].shape
    F = len(fields)
    Bc = send.shape[2] if send.dim() == 5 else -1
    if not (send.is_cuda and send.is_contiguous() and send.dtype == fields[0].dtype and ny % P == 0 and tuple(send.shape) == (P, F, Bc, nloc, ny // P) and 0 <= g0 and g0 + Bc <= B):
        raise ValueError("slab_pack_halo: send must be [%d, %d, Bc, %d, %d] with g0 + Bc <= %d" % (P, F, nloc, ny // P, B))
    for h in (first, last):
        if h is not None and not (h.is_cuda and h.is_contiguous() and h.dtype == fields[0].dtype and tuple(h.shape) == (F, B, ny)):
            raise ValueError("slab_pack_halo: first / last must be contiguous [%d, %d, %d]" % (F, B, ny))
    _call('nns_slab_pack_halo', suf, _ptr_array(fields), F, _p(send), _p(first) if first is not None else None, _p(last) if last is not None else None,
          B, int(g0), Bc, nloc, ny, P, _stream())
    return send


def slab_transpose_unpack(recv, fields, P):
    """recv [P, F, B, nloc, ny / P] -> row slabs fields[f] [B, nloc, ny] (nns_slab_transpose_unpack_*)."""
    suf = _slab_fields(fields, 'slab_transpose_unpack')
    B, nloc, ny = fields[0].shape
    if not (recv.is_cuda and recv.is_contiguous() and recv.dtype == fields[0].dtype and tuple(recv.shape) == (P, len(fields), B, nloc, ny // P) and ny % P == 0):
        raise ValueError("slab_transpose_unpack: recv must be [%d, %d, %d, %d, %d]" % (P, len(fields), B, nloc, ny // P))
    _call('nns_slab_transpose_unpack', suf, _p(recv), _ptr_array(fields), len(fields), B, nloc, ny, P, _stream())
    return fields


def spec_residual_ypass_(u, v, p, u_prev, v_prev, ru, rv, rd, dt, Ly, rho, nu, precise=True):
    suf, (B, nx, ny) = _chk(u, v, p, u_prev, v_prev, ru, rv, rd)
    if suf != '_f32':
        raise TypeError("spec_residual_ypass: float32 fields")
    check(_lib.lib().nns_spec_residual_ypass_f32(_p(u), _p(v), _p(p), _p(u_prev), _p(v_prev), _p(ru), _p(rv), _p(rd), B, nx, ny,
                                                 dt, Ly, rho, nu, _prec(precise), _stream()), 'nns_spec_residual_ypass_f32')
    return ru, rv, rd


# ----------------------------------------------------------------------------- neural_spectral
ODE_METHODS = {'Euler': 0, 'RK2': 1, 'RK4': 2}


def _f32(*ts):
    for t in ts:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise TypeError("expected contiguous float32 CUDA/HIP tensors")


def ode_mlp_fwd(z0, W0, b0, W1, b1, W2, b2, Nt, method):
    _f32(z0, W0, b0, W1, b1, W2, b2)
    mb, K = z0.shape
    out = torch.empty(Nt, mb, K, dtype=torch.float32, device=z0.device)
    check(_lib.lib().nns_ode_mlp_fwd_f32(_p(z0), _p(W0), _p(b0), _p(W1), _p(b1), _p(W2), _p(b2), _p(out), mb, K, W1.shape[0],
                                         int(Nt), ODE_METHODS[method], _stream()), 'nns_ode_mlp_fwd_f32')
    return out


def ode_mlp_bwd(z0, W0, b0, W1, b1, W2, b2, states, grad_out, Nt, method):
    _f32(z0, W0, b0, W1, b1, W2, b2, states, grad_out)
    mb, K = z0.shape
    gz0 = torch.empty_like(z0)
    gs = [torch.empty_like(t) for t in (W0, b0, W1, b1, W2, b2)]
    work = torch.empty(_lib.lib().nns_ode_mlp_bwd_workspace(mb) // 4, dtype=torch.float32, device=z0.device)
    check(_lib.lib().nns_ode_mlp_bwd_f32(_p(z0), _p(W0), _p(b0), _p(W1), _p(b1), _p(W2), _p(b2), _p(states), _p(grad_out), _p(gz0),
                                         *[_p(g) for g in gs], _p(work), mb, K, W1.shape[0], int(Nt), ODE_METHODS[method], _stream()),
          'nns_ode_mlp_bwd_f32')
    return gz0, gs


def ode_mlp_bwd_steps(y, W0, b0, W1, b1, W2, b2, grad_out, dt, method, want_param_grads=True):
    """Backward of rows INDEPENDENT single steps of size dt (nns_ode_mlp_bwd_steps_f32): returns (grad_y [rows, K], parameter
    gradients summed over the rows -- None with want_param_grads=False: the kernel then skips their products, memsets and atomics)."""
    _f32(y, W0, b0, W1, b1, W2, b2, grad_out)
    rows, K = y.shape
    gy = torch.empty_like(y)
    gs = [torch.empty_like(t) for t in (W0, b0, W1, b1, W2, b2)] if want_param_grads else None
    work = torch.empty(_lib.lib().nns_ode_mlp_bwd_workspace(rows) // 4, dtype=torch.float32, device=y.device)
    check(_lib.lib().nns_ode_mlp_bwd_steps_f32(_p(y), _p(W0), _p(b0), _p(W1), _p(b1), _p(W2), _p(b2), _p(grad_out), _p(gy),
                                               *([_p(g) for g in gs] if want_param_grads else [None] * 6), _p(work), rows, K, W1.shape[0], float(dt),
                                               ODE_METHODS[method], _stream()),
          'nns_ode_mlp_bwd_steps_f32')
    return gy, gs


def ode_adjoint_chain(J, g):
    """lam[Nt-1] = g[Nt-1], lam[s-1] = g[s-1] + lam[s] @ J[s] for J [Nt, mb, K, K], g [Nt, mb, K] (nns_ode_adjoint_chain_f32)."""
    _f32(J, g)
    Nt, mb, K = g.shape
    lam = torch.empty_like(g)
    check(_lib.lib().nns_ode_adjoint_chain_f32(_p(J), _p(g), _p(lam), Nt, mb, K, _stream()), 'nns_ode_adjoint_chain_f32')
    return lam


def basis_expand(coeff, basis):
    """coeff [T, K, C], basis [K, C, P] -> pred [T, C, P]"""
    _f32(coeff, basis)
    T, K, C = coeff.shape
    P = basis.shape[2]
    pred = torch.empty(T, C, P, dtype=torch.float32, device=coeff.device)
    check(_lib.lib().nns_basis_expand_f32(_p(coeff), _p(basis), _p(pred), T, K, C, P, _stream()), 'nns_basis_expand_f32')
    return pred


def basis_expand_bwd(coeff, basis, grad_pred):
    _f32(coeff, basis, grad_pred)
    T, K, C = coeff.shape
    P = basis.shape[2]
    gc, gb = torch.empty_like(coeff), torch.empty_like(basis)
    check(_lib.lib().nns_basis_expand_bwd_f32(_p(coeff), _p(basis), _p(grad_pred), _p(gc), _p(gb), T, K, C, P, _stream()), 'nns_basis_expand_bwd_f32')
    return gc, gb


def basis_loss_fwd(coeff, basis, obs):
    """sum (pred - obs)^2 as a device float64 scalar tensor (pred never materialised)."""
    _f32(coeff, basis, obs)
    T, K, C = coeff.shape
    P = basis.shape[2]
    ss = torch.zeros(1, dtype=torch.float64, device=coeff.device)
    check(_lib.lib().nns_basis_loss_fwd_f32(_p(coeff), _p(basis), _p(obs), _p(ss), T, K, C, P, _stream()), 'nns_basis_loss_fwd_f32')
    return ss


def basis_loss_fused(coeff, basis, obs):
    """ONE sweep over obs: returns (sumsq float64 device scalar, d(sumsq/2)/dcoeff, d(sumsq/2)/dbasis) -- the gradient without the
    upstream / loss factor (nns_basis_loss_fused_f32)."""
    _f32(coeff, basis, obs)
    T, K, C = coeff.shape
    P = basis.shape[2]
    ss = torch.zeros(1, dtype=torch.float64, device=coeff.device)
    gc, gb = torch.empty_like(coeff), torch.empty_like(basis)
    check(_lib.lib().nns_basis_loss_fused_f32(_p(coeff), _p(basis), _p(obs), _p(ss), _p(gc), _p(gb), T, K, C, P, _stream()), 'nns_basis_loss_fused_f32')
    return ss, gc, gb


def basis_loss_bwd(coeff, basis, obs, scale):
    _f32(coeff, basis, obs)
    T, K, C = coeff.shape
    P = basis.shape[2]
    gc, gb = torch.empty_like(coeff), torch.empty_like(basis)
    check(_lib.lib().nns_basis_loss_bwd_f32(_p(coeff), _p(basis), _p(obs), float(scale), _p(gc), _p(gb), T, K, C, P, _stream()), 'nns_basis_loss_bwd_f32')
    return gc, gb


# ----------------------------------------------------------------------------- chorin_spectral
def _f64(*ts):
    for t in ts:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()):
            raise TypeError("expected contiguous float64 CUDA/HIP tensors")


def cheb_gemm(A, B, transA=False, transB=False, alpha=1.0, beta=0.0, out=None):
    """Row-major 2-D float64: out = alpha * op(A) @ op(B) + beta * out."""
    _f64(A, B)
    M = A.shape[1] if transA else A.shape[0]
    K = A.shape[0] if transA else A.shape[1]
    N = B.shape[0] if transB else B.shape[1]
    if (B.shape[1] if transB else B.shape[0]) != K:
        raise ValueError("cheb_gemm: inner dimensions differ")
    if out is None:
        out = torch.empty(M, N, dtype=torch.float64, device=A.device)
        beta = 0.0
    _f64(out)
    check(_lib.lib().nns_cheb_gemm_f64(_p(A), A.shape[1], int(transA), _p(B), B.shape[1], int(transB), _p(out), out.shape[1],
                                       M, N, K, float(alpha), float(beta), 1, _stream()), 'nns_cheb_gemm_f64')
    return out


def cheb_helmholtz_rhs(f, un, vn, un1, vn1, fx, fy, f1x, f1y, fxx, fyy, dt):
    _f64(f, un, vn, un1, vn1, fx, fy, f1x, f1y, fxx, fyy)
    F = torch.empty_like(f)
    check(_lib.lib().nns_cheb_helmholtz_rhs_f64(*[_p(t) for t in (f, un, vn, un1, vn1, fx, fy, f1x, f1y, fxx, fyy)], _p(F), f.numel(),
                                                float(dt), _stream()), 'nns_cheb_helmholtz_rhs_f64')
    return F


def cheb_diag_div(Hm, lam_x, lam_y, c0, cx, cy):
    _f64(Hm, lam_x, lam_y)
    out = torch.empty_like(Hm)
    check(_lib.lib().nns_cheb_diag_div_f64(_p(Hm), _p(lam_x), _p(lam_y), _p(out), Hm.shape[0], Hm.shape[1], float(c0), float(cx), float(cy),
                                           _stream()), 'nns_cheb_diag_div_f64')
    return out


def cheb_embed(sol, x0, xN, y0, yN):
    _f64(sol, x0, xN, y0, yN)
    Nx, Ny = sol.shape[0] + 2, sol.shape[1] + 2
    full = torch.empty(Nx, Ny, dtype=torch.float64, device=sol.device)
    check(_lib.lib().nns_cheb_embed_f64(_p(sol), _p(x0), _p(xN), _p(y0), _p(yN), _p(full), Nx, Ny, _stream()), 'nns_cheb_embed_f64')
    return full


# ----------------------------------------------------------------------------- per-pixel MLP (BasisFunc)
def pixel_mlp_fwd(x, weights, biases, bf16=False):
    """x [mb, C_in, nx, ny] (or [mb, C_in, P]); weights: list of [C_out, C_in] (or Conv2d [C_out, C_in, 1, 1]) tensors;
    biases: list of [C_out].  ReLU between layers, none after the last."""
    mb, P, ws, widths, wp, bp = _pixel_mlp_pack(x, weights, biases, 'pixel_mlp_fwd')
    y = torch.empty((mb, widths[-1]) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
    arr = (ctypes.c_int * len(widths))(*widths)
    check(_lib.lib().nns_pixel_mlp_fwd_f32(_p(x), _p(wp), _p(bp), _p(y), mb, P, arr, len(ws), int(bool(bf16)), _stream()), 'nns_pixel_mlp_fwd_f32')
    return y


def _pixel_mlp_pack(x, weights, biases, what):
    _f32(x)
    mb, cin = x.shape[0], x.shape[1]
    P = x[0, 0].numel()
    ws = [w.reshape(w.shape[0], w.shape[1]) for w in weights]
    widths = [cin] + [w.shape[0] for w in ws]
    for i, w in enumerate(ws):
        if w.shape[1] != widths[i]:
            raise ValueError("%s: layer %d expects %d input channels, got %d" % (what, i, w.shape[1], widths[i]))
    wp = torch.cat([w.reshape(-1) for w in ws]).to(torch.float32).contiguous()
    bp = torch.cat([b.reshape(-1) for b in biases]).to(torch.float32).contiguous()
    return mb, P, ws, widths, wp, bp


def pixel_mlp_bwd(x, gy, weights, biases, bf16=True, out=None, workspace=None):
    """Backward of pixel_mlp_fwd: returns (gx like x, [gW_l like weights[l]], [gb_l like biases[l]]).
    bf16=False (float32 operands) supports widths <= 32.
    out: (gx like x, gW and gB packed like the weights and the biases) to write into instead of new tensors -- overwritten, not accumulated;
    workspace: a contiguous tensor to use as scratch, whatever it holds (nns_pixel_mlp_bwd_workspace bytes at least: a smaller one is an error)."""
    mb, P, ws, widths, wp, bp = _pixel_mlp_pack(x, weights, biases, 'pixel_mlp_bwd')
    _f32(gy)
    if tuple(gy.shape) != (mb, widths[-1]) + tuple(x.shape[2:]):
        raise ValueError("pixel_mlp_bwd: gy has shape %s, expected %s" % (tuple(gy.shape), (mb, widths[-1]) + tuple(x.shape[2:])))
    arr = (ctypes.c_int * len(widths))(*widths)
    if workspace is None:
        nbytes = _query_bytes('nns_pixel_mlp_bwd_workspace', arr, len(ws))
        work = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=x.device)
    else:
        if not (workspace.is_cuda and workspace.is_contiguous()):
            raise TypeError("pixel_mlp_bwd: workspace must be a contiguous CUDA/HIP tensor")
        work, nbytes = workspace, workspace.numel() * workspace.element_size()
    if out is None:
        gx, gW, gB = torch.empty_like(x), torch.empty_like(wp), torch.empty_like(bp)
    else:
        gx, gW, gB = out
        _f32(gx, gW, gB)
        if gx.shape != x.shape or gW.shape != wp.shape or gB.shape != bp.shape:
            raise ValueError("pixel_mlp_bwd: out must be (gx like x, gW [%d], gB [%d])" % (wp.numel(), bp.numel()))
    check(_lib.lib().nns_pixel_mlp_bwd_f32(_p(x), _p(gy), _p(wp), _p(bp), _p(gx), _p(gW), _p(gB), mb, P, arr, len(ws), int(bool(bf16)),
                                           _p(work), nbytes, _stream()), 'nns_pixel_mlp_bwd_f32')
    gws, gbs, wo, bo = [], [], 0, 0
    for w, b in zip(weights, biases):
        gws.append(gW[wo:wo + w.numel()].reshape(w.shape)); wo += w.numel()
        gbs.append(gB[bo:bo + b.numel()].reshape(b.shape)); bo += b.numel()
    return gx, gws, gbs


class PixelMlpFn(torch.autograd.Function):
    """pixel_mlp_fwd / pixel_mlp_bwd as one autograd node (bf16 or float32 operands, float32 accumulation)."""

    @staticmethod
    def forward(ctx, x, nlayers, bf16, *params):
        weights, biases = params[:nlayers], params[nlayers:]
        ctx.nlayers, ctx.bf16 = nlayers, bool(bf16)
        x = x.contiguous()
        ctx.save_for_backward(x, *params)
        return pixel_mlp_fwd(x, weights, biases, bf16=bf16)

    @staticmethod
    def backward(ctx, gy):
        x, *params = ctx.saved_tensors
        weights, biases = params[:ctx.nlayers], params[ctx.nlayers:]
        gx, gws, gbs = pixel_mlp_bwd(x.contiguous(), gy.contiguous(), weights, biases, bf16=ctx.bf16)
        return (gx, None, None) + tuple(gws) + tuple(gbs)


# ----------------------------------------------------------------------------- standalone spectral operators
def spec_derivs(f, Lx, Ly, want=('x', 'y', 'lap'), precise=True):
    """Spectral f_x, f_y, lap f of one real float32 field [B, nx, ny] (or [nx, ny]); returns a dict."""
    _f32(f)
    B, nx, ny = _dims(f)
    out = {k: torch.empty_like(f) for k in want}
    ptr = lambda k: _p(out[k]) if k in out else None
    check(_lib.lib().nns_spec_derivs_f32(_p(f), ptr('x'), ptr('y'), ptr('lap'), B, nx, ny, float(Lx), float(Ly), _prec(precise), _stream()),
          'nns_spec_derivs_f32')
    return out


def spec_residual_bwd(u, v, g_u, g_v, g_div, dt, Lx, Ly, rho, nu, precise=True, want_prev=True):
    """Vector-Jacobian product of spec_residual (oracle/periodic.py: spectral_residual_vjp) by the fused two-pass
    backward kernels (nns_spec_residual_bwd_f32): returns (grad_u, grad_v, grad_p, grad_u_prev, grad_v_prev)."""
    suf, (B, nx, ny) = _chk(u, v, g_u, g_v, g_div)
    if suf != '_f32':
        raise TypeError("spec_residual_bwd: float32 fields")
    gu, gv, gp = torch.empty_like(u), torch.empty_like(u), torch.empty_like(u)
    gup, gvp = (torch.empty_like(u), torch.empty_like(u)) if want_prev else (None, None)
    check(_lib.lib().nns_spec_residual_bwd_f32(_p(u), _p(v), _p(g_u), _p(g_v), _p(g_div), _p(gu), _p(gv), _p(gp),
                                               _p(gup) if want_prev else None, _p(gvp) if want_prev else None,
                                               B, nx, ny, dt, Lx, Ly, rho, nu, _prec(precise), _stream()), 'nns_spec_residual_bwd_f32')
    return gu, gv, gp, gup, gvp


def spec_residual_bwd_composed(u, v, g_u, g_v, g_div, dt, Lx, Ly, rho, nu, precise=True):
    """The same product assembled from the standalone spectral-derivative kernel (8 launches) and elementwise tensor
    ops: kept as an independent cross-check of the fused kernels (tests), not used on the training path."""
    _f32(u, v, g_u, g_v, g_div)
    d = lambda f, *want: spec_derivs(f.contiguous(), Lx, Ly, want, precise)
    du, dv = d(u, 'x', 'y'), d(v, 'x', 'y')
    da, db = d(g_u, 'x', 'lap'), d(g_v, 'y', 'lap')
    grad_u = g_u / dt + g_u * du['x'] + g_v * dv['x'] - d(g_u * u + g_div, 'x')['x'] - d(g_u * v, 'y')['y'] - nu * da['lap']
    grad_v = g_v / dt + g_u * du['y'] + g_v * dv['y'] - d(g_v * u, 'x')['x'] - d(g_v * v + g_div, 'y')['y'] - nu * db['lap']
    grad_p = -(da['x'] + db['y']) / rho
    return grad_u, grad_v, grad_p


class SpecResidualFn(torch.autograd.Function):
    """spec_residual as an autograd node."""

    @staticmethod
    def forward(ctx, u, v, p, u_prev, v_prev, dt, Lx, Ly, rho, nu, precise):
        u, v, p, u_prev, v_prev = (t.contiguous() for t in (u, v, p, u_prev, v_prev))
        ctx.save_for_backward(u, v)
        ctx.consts = (dt, Lx, Ly, rho, nu, precise)
        return spec_residual(u, v, p, u_prev, v_prev, dt, Lx, Ly, rho, nu, precise)

    @staticmethod
    def backward(ctx, g_u, g_v, g_d):
        u, v = ctx.saved_tensors
        dt, Lx, Ly, rho, nu, precise = ctx.consts
        zero = lambda g: torch.zeros_like(u) if g is None else g.contiguous()
        want_prev = ctx.needs_input_grad[3] or ctx.needs_input_grad[4]
        return spec_residual_bwd(u, v, zero(g_u), zero(g_v), zero(g_d), dt, Lx, Ly, rho, nu, precise, want_prev) + (None,) * 6


def spec_rfft2(f):
    """numpy.fft.rfft2 of float32 [B, nx, ny] -> complex64 [B, nx, ny//2+1]."""
    _f32(f)
    B, nx, ny = _dims(f)
    spec = torch.empty((B, nx, ny // 2 + 1, 2), dtype=torch.float32, device=f.device)
    check(_lib.lib().nns_spec_rfft2_f32(_p(f), _p(spec), B, nx, ny, _stream()), 'nns_spec_rfft2_f32')
    return torch.view_as_complex(spec)


def spec_irfft2(spec, ny):
    """numpy.fft.irfft2(spec, s=(nx, ny)) for complex64 [B, nx, ny//2+1]; the input is not modified (a scratch copy is)."""
    s = torch.view_as_real(spec.contiguous()).clone()
    _f32(s)
    B, nx = spec.shape[0], spec.shape[1]
    f = torch.empty((B, nx, ny), dtype=torch.float32, device=spec.device)
    check(_lib.lib().nns_spec_irfft2_f32(_p(s), _p(f), B, nx, ny, _stream()), 'nns_spec_irfft2_f32')
    return f


# ----------------------------------------------------------------------------- pseudo-spectral periodic solver (nns_spec_ns_*)
def spec_ns_kept_y(ny):
    """Kept y-wavenumbers of the 2/3 rule: j < (ny - 1) // 3 + 1."""
    return (int(ny) - 1) // 3 + 1


def spec_ns_workspace(B, nx, ny):
    """Bytes of the workspace nns_spec_ns_init / step / fields need for B grids of nx x ny."""
    return _query_bytes('nns_spec_ns_workspace', int(B), int(nx), int(ny))


def _spec_ns_work(who, work):
    if not (isinstance(work, torch.Tensor) and work.is_cuda and work.dtype == torch.uint8 and work.is_contiguous()):
        raise TypeError("%s: work must be a contiguous uint8 device tensor" % who)


def _spec_ns_out(who, out, shape, device):
    """The float64 result of `shape` on the state's device: a fresh one (out None) or the checked out."""
    if out is None:
        return torch.empty(shape, dtype=torch.float64, device=device)
    if not (isinstance(out, torch.Tensor) and out.dtype == torch.float64 and tuple(out.shape) == shape and out.is_contiguous()
            and out.device == device):
        raise ValueError("%s: out must be a contiguous float64 %s tensor on the state's device" % (who, list(shape)))
    return out


def _spec_ns_field_out(who, out, shape, device, three=True):
    """Its float32 twin for the physical fields: a tuple of three of `shape`, or (three False) one bare tensor."""
    n = 3 if three else 1
    if out is None:
        out = tuple(torch.empty(shape, dtype=torch.float32, device=device) for _ in range(n))
    else:
        out = tuple(out) if three else (out,)
        _f32(*out)
        if len(out) != n or any(tuple(o.shape) != shape or o.device != device for o in out):
            raise ValueError("%s: out must be %s %s tensor%s on the state's device" % (who, "three" if three else "a", list(shape), "s" if three else ""))
    return out if three else out[0]


def _spec_ns_state(who, what, mean, work, ny):
    """(B, my1, nx) of the checked solver state.  mean and work None (spec_ns_diag): the spectrum alone, under the caller's name; ny None
    (spec_ns_init, which compares the whole shape with its fields): no check of the kept y-wavenumbers."""
    alone = mean is None
    _f32(*((what,) if alone else (what, mean)))
    if what.dim() != 4 or what.shape[3] != 2:
        raise ValueError("%s: what must be float32 [B, my1, nx, 2], got %s" % (who if alone else 'spec_ns', tuple(what.shape)))
    B, my1, nx = what.shape[0], what.shape[1], what.shape[2]
    if not alone:
        if tuple(mean.shape) != (B, 2):
            raise ValueError("spec_ns: mean must be [B, 2], got %s" % (tuple(mean.shape),))
        _spec_ns_work('spec_ns', work)
        if what.device != mean.device or what.device != work.device:
            raise ValueError("spec_ns: state tensors on different devices")
    if ny is not None and my1 != spec_ns_kept_y(ny):
        raise ValueError("%s: what has %d kept y-wavenumbers, ny = %d needs %d" % (who, my1, ny, spec_ns_kept_y(ny)))
    return B, my1, nx


def spec_ns_init(u, v, what, mean, work, Lx, Ly):
    """what, mean <- the solver state of velocity (u, v) [B, nx, ny] float32: what = M (i kx v^ - i ky u^) compacted ([B, my1, nx, 2]),
    mean = the grid means [B, 2].  Divergence-free, band-limited projection of the input."""
    _f32(u, v)
    suf, (B, nx, ny) = _chk(u, v)
    Bw, my1, nxw = _spec_ns_state('spec_ns_init', what, mean, work, None)
    if (Bw, my1, nxw) != (B, spec_ns_kept_y(ny), nx) or u.device != what.device:
        raise ValueError("spec_ns_init: state [%d, %d, %d] does not match fields [%d, %d, %d]" % (Bw, my1, nxw, B, nx, ny))
    check(_lib.lib().nns_spec_ns_init_f32(_p(u), _p(v), _p(what), _p(mean), _p(work), work.numel(), B, nx, ny, float(Lx), float(Ly),
                                          _stream()), 'nns_spec_ns_init_f32')
    return what, mean


def _pn(t):
    """t's device pointer; None (NULL) for None."""
    return None if t is None else t.data_ptr()


def _spec_ns_f32(who, name, t, shape, device):
    """t is a contiguous float32 tensor of `shape` on the state's device."""
    _f32(t)
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s: %s must be float32 %s, got %s" % (who, name, list(shape), tuple(t.shape)))
    if t.device != device:
        raise ValueError("%s: %s must be on the state's device %s" % (who, name, device))


_ABSENT = object()                 # in place of an argument that a C entry does not have (None is a NULL it does have)


def _spec_ns_step(entry, what, mean, work, ny, Lx, Ly, dt, numbers, nsteps, that=_ABSENT, ghat=_ABSENT, lin=_ABSENT, noise=_ABSENT,
                  optional=(), dwhat=_ABSENT, dthat=_ABSENT, members=False, dghat=_ABSENT):
    """Every forward step, the tangent ones included: the checks of the tensors, then the call of `entry`, whose arguments are what, [that,]
    [dwhat, [dthat,] [K,]] mean, [ghat, gbatch, [dghat, dgbatch,]] work, its size, the box and dt, `numbers` (the entry's doubles after dt),
    [lin,] [amp, seed, clock, ids,] nsteps and the stream.  that, dwhat, dthat, ghat, dghat, lin, noise = (amp, seed, clock, ids): the
    bracketed ones the entry has; `members`: dwhat and dthat are K members, [K, B, my1, nx, 2] (_spec_ns_tangents), and K is an argument;
    `optional` names those of 'that', 'lin' and 'noise' it takes as NULL (that None; lin None; amp, clock and ids all None); noise None,
    the tangent steps' way to say no noise, is four NULLs.  The caller's name in the messages is the entry's without nns_ and f32."""
    who = entry[4:-3]
    B, my1, nx = _spec_ns_state(who, what, mean, work, ny)
    args = [_p(what)]
    if that is not _ABSENT:
        if that is not None or 'that' not in optional:
            _spec_ns_same(who, that, what)
        args.append(_pn(that))
    if dwhat is not _ABSENT:
        if members:
            K = _spec_ns_tangents(who, dwhat, ny, B, my1, nx, what.device)[0]
        else:
            _spec_ns_same(who, dwhat, what, 'dwhat')
        args.append(_p(dwhat))
        if dthat is not _ABSENT:
            _spec_ns_same(who, dthat, dwhat, 'dthat')
            args.append(_p(dthat))
        if members:
            args.append(K)
    args.append(_p(mean))
    if ghat is not _ABSENT:
        args += (_pn(ghat), _spec_ns_force(who, ghat, what))
    if dghat is not _ABSENT:
        args += (_pn(dghat), _spec_ns_force(who, dghat, what))
    args += (_p(work), work.numel(), B, nx, int(ny), float(Lx), float(Ly), float(dt))
    args.extend(map(float, numbers))
    if lin is not _ABSENT:
        if lin is not None or 'lin' not in optional:
            _spec_ns_f32(who, 'lin', lin, (my1, nx, 2), what.device)
        args.append(_pn(lin))
    if noise is not _ABSENT:
        amp, seed, clock, ids = noise or (None, 0, None, None)
        if 'noise' in optional and (amp is None or clock is None or ids is None):
            if not (amp is None and clock is None and ids is None):
                raise ValueError("%s: amp, clock and ids must be all None (no noise) or all given" % who)
        elif noise is not None:
            _spec_ns_noise(who, amp, seed, clock, ids, B, my1, nx, what.device)
        args += (_pn(amp), int(seed), _pn(clock), _pn(ids))
    check(getattr(_lib.lib(), entry)(*args, int(nsteps), _stream()), entry)
    return what


def spec_ns_step_(what, mean, work, ny, Lx, Ly, dt, nu, nsteps=1):
    """nsteps Lawson-RK4 steps on what in place (no allocation, no host synchronisation: capturable)."""
    return _spec_ns_step('nns_spec_ns_step_f32', what, mean, work, ny, Lx, Ly, dt, (nu,), nsteps)


def spec_ns_fields(what, mean, work, ny, Lx, Ly, rho, out=None):
    """(u, v, p) float32 [B, nx, ny] of the state; out: three preallocated contiguous tensors of that shape."""
    B, my1, nx = _spec_ns_state('spec_ns_fields', what, mean, work, ny)
    u, v, p = out = _spec_ns_field_out('spec_ns_fields', out, (B, nx, int(ny)), what.device)
    check(_lib.lib().nns_spec_ns_fields_f32(_p(what), _p(mean), _p(u), _p(v), _p(p), _p(work), work.numel(), B, nx, int(ny), float(Lx),
                                            float(Ly), float(rho), _stream()), 'nns_spec_ns_fields_f32')
    return out


def _spec_ns_force(who, ghat, what):
    """gbatch of the force spectrum ghat (None: 0) for the state what: float32 [1 or B, my1, nx, 2] on what's device."""
    if ghat is None:
        return 0
    _f32(ghat)
    B = what.shape[0]
    if ghat.dim() != 4 or tuple(ghat.shape[1:]) != tuple(what.shape[1:]) or ghat.shape[0] not in (1, B):
        raise ValueError("%s: ghat must be float32 [1 or %d, %d, %d, 2], got %s" % (who, B, what.shape[1], what.shape[2], tuple(ghat.shape)))
    if ghat.device != what.device:
        raise ValueError("%s: ghat is on %s, the state on %s" % (who, ghat.device, what.device))
    return int(ghat.shape[0])


def spec_ns_step_forced_(what, mean, ghat, work, ny, Lx, Ly, dt, nu, drag, nsteps=1):
    """nsteps Lawson-RK4 steps with the force spectrum ghat ([1, my1, nx, 2]: shared by the batch, [B, my1, nx, 2]: one per grid, None: no
    force) and the linear drag `drag` on what in place (no allocation, no host synchronisation: capturable)."""
    return _spec_ns_step('nns_spec_ns_step_forced_f32', what, mean, work, ny, Lx, Ly, dt, (nu, drag), nsteps, ghat=ghat)


def spec_ns_diag(what, ghat, ny, Lx, Ly, out=None):
    """float64 [B, 3]: fluctuation energy, enstrophy and power input <f_s . u> (0 with ghat None) of every grid of the state."""
    B, my1, nx = _spec_ns_state('spec_ns_diag', what, None, None, ny)
    gbatch = _spec_ns_force('spec_ns_diag', ghat, what)
    out = _spec_ns_out('spec_ns_diag', out, (B, 3), what.device)
    check(_lib.lib().nns_spec_ns_diag_f32(_p(what), _pn(ghat), gbatch, _p(out), B, nx, int(ny), float(Lx), float(Ly),
                                          _stream()), 'nns_spec_ns_diag_f32')
    return out


# passive scalar of the periodic solver (nns_spec_ns_scalar_*, and its step)
def spec_ns_scalar_workspace(B, nx, ny):
    """Bytes of the workspace the scalar calls need for B grids of nx x ny (>= spec_ns_workspace: it serves every spec_ns call)."""
    return _query_bytes('nns_spec_ns_scalar_workspace', int(B), int(nx), int(ny))


def _spec_ns_scalar(who, that, work, ny):
    """(B, my1, nx) of the checked scalar spectrum that (float32 [B, my1, nx, 2]) and, unless None, its workspace."""
    _f32(that)
    if that.dim() != 4 or that.shape[3] != 2:
        raise ValueError("%s: that must be float32 [B, my1, nx, 2], got %s" % (who, tuple(that.shape)))
    B, my1, nx = that.shape[0], that.shape[1], that.shape[2]
    if my1 != spec_ns_kept_y(ny):
        raise ValueError("%s: that has %d kept y-wavenumbers, ny = %d needs %d" % (who, my1, ny, spec_ns_kept_y(ny)))
    if work is not None:
        _spec_ns_work(who, work)
        if work.device != that.device:
            raise ValueError("%s: state tensors on different devices" % who)
    return B, my1, nx


def spec_ns_scalar_init(theta, that, work):
    """that <- M_theta rfft2(theta) compacted ([B, my1, nx, 2]) for theta [B, nx, ny] float32: its band-limited part, the mean included."""
    _f32(theta)
    suf, (B, nx, ny) = _chk(theta)
    if (B, spec_ns_kept_y(ny), nx) != _spec_ns_scalar('spec_ns_scalar_init', that, work, ny) or theta.device != that.device:
        raise ValueError("spec_ns_scalar_init: state %s does not match the field [%d, %d, %d]" % (tuple(that.shape), B, nx, ny))
    check(_lib.lib().nns_spec_ns_scalar_init_f32(_p(theta), _p(that), _p(work), work.numel(), B, nx, ny, _stream()),
          'nns_spec_ns_scalar_init_f32')
    return that


def spec_ns_scalar_field(that, work, ny, out=None):
    """theta float32 [B, nx, ny] of the scalar state; out: a preallocated contiguous tensor of that shape."""
    B, my1, nx = _spec_ns_scalar('spec_ns_scalar_field', that, work, ny)
    out = _spec_ns_field_out('spec_ns_scalar_field', out, (B, nx, int(ny)), that.device, three=False)
    check(_lib.lib().nns_spec_ns_scalar_field_f32(_p(that), _p(out), _p(work), work.numel(), B, nx, int(ny), _stream()),
          'nns_spec_ns_scalar_field_f32')
    return out


def _spec_ns_same(who, that, what, name='that'):
    """that (under `name` in the messages) is a spectrum like what."""
    _spec_ns_f32(who, name, that, what.shape, what.device)


def spec_ns_step_scalar_(what, that, mean, ghat, work, ny, Lx, Ly, dt, nu, drag, kappa, grad=(0.0, 0.0), nsteps=1):
    """nsteps Lawson-RK4 steps of the flow and its passive scalar, (what, that) in place: diffusivity kappa, uniform mean gradient grad =
    (Gx, Gy); ghat and drag as in spec_ns_step_forced_ (None and 0: the unforced flow).  what comes out bitwise as without the scalar.
    work: spec_ns_scalar_workspace bytes.  No allocation, no host synchronisation: capturable."""
    return _spec_ns_step('nns_spec_ns_step_scalar_f32', what, mean, work, ny, Lx, Ly, dt, (nu, drag, kappa, *grad), nsteps, that=that,
                         ghat=ghat), that


def spec_ns_scalar_diag(what, that, ny, Lx, Ly, kappa, out=None):
    """float64 [B, 4]: variance 1/2 <theta'^2>, dissipation kappa <|grad theta|^2> and the fluxes <u theta'>, <v theta'> of every grid."""
    B, my1, nx = _spec_ns_state('spec_ns_scalar_diag', what, None, None, ny)
    _spec_ns_same('spec_ns_scalar_diag', that, what)
    out = _spec_ns_out('spec_ns_scalar_diag', out, (B, 4), what.device)
    check(_lib.lib().nns_spec_ns_scalar_diag_f32(_p(what), _p(that), _p(out), B, nx, int(ny), float(Lx), float(Ly), float(kappa), _stream()),
          'nns_spec_ns_scalar_diag_f32')
    return out


# shell spectra and spectral transfers of the periodic solver (nns_spec_ns_shells, nns_spec_ns_spectrum_f32, nns_spec_ns_transfer_f32)
def spec_ns_shells(nx, ny, Lx, Ly):
    """(nshell, dk) of the box: shells of width dk = min(2 pi / Lx, 2 pi / Ly) centred on s dk, s = 0 .. nshell - 1 (host only)."""
    n, dk = ctypes.c_int(0), ctypes.c_double(0.0)
    check(_lib.lib().nns_spec_ns_shells(int(nx), int(ny), float(Lx), float(Ly), ctypes.byref(n), ctypes.byref(dk)), 'nns_spec_ns_shells')
    return n.value, dk.value


def spec_ns_spectrum(what, that, ghat, ny, Lx, Ly, out=None):
    """float64 [B, 4, nshell]: per grid and shell the energy, enstrophy, injection Re(psi^ conj g^) (zeros with ghat None) and scalar variance
    (zeros with that None); their sums over the shells are spec_ns_diag's and spec_ns_scalar_diag's numbers."""
    B, my1, nx = _spec_ns_state('spec_ns_spectrum', what, None, None, ny)
    if that is not None:
        _spec_ns_same('spec_ns_spectrum', that, what)
    gbatch = _spec_ns_force('spec_ns_spectrum', ghat, what)
    S = spec_ns_shells(nx, ny, Lx, Ly)[0]
    out = _spec_ns_out('spec_ns_spectrum', out, (B, 4, S), what.device)
    check(_lib.lib().nns_spec_ns_spectrum_f32(_p(what), _pn(that), _pn(ghat), gbatch, _p(out), S, B,
                                              nx, int(ny), float(Lx), float(Ly), _stream()), 'nns_spec_ns_spectrum_f32')
    return out


def spec_ns_transfer(what, that, work, ny, Lx, Ly, out=None):
    """float64 [B, 3, nshell]: the nonlinear transfer of energy, enstrophy and scalar variance (zeros with that None) into every shell, from
    one evaluation of the step's nonlinear term in the co-moving frame.  what and that are only read; work: spec_ns_workspace bytes
    (spec_ns_scalar_workspace with that).  No allocation beyond out, no host synchronisation: capturable with out given."""
    _spec_ns_work('spec_ns_transfer', work)
    B, my1, nx = _spec_ns_state('spec_ns_transfer', what, None, None, ny)
    if work.device != what.device:
        raise ValueError("spec_ns_transfer: state tensors on different devices")
    if that is not None:
        _spec_ns_same('spec_ns_transfer', that, what)
    S = spec_ns_shells(nx, ny, Lx, Ly)[0]
    out = _spec_ns_out('spec_ns_transfer', out, (B, 3, S), what.device)
    check(_lib.lib().nns_spec_ns_transfer_f32(_p(what), _pn(that), _p(out), S, _p(work), work.numel(), B, nx, int(ny),
                                              float(Lx), float(Ly), _stream()), 'nns_spec_ns_transfer_f32')
    return out


# Boussinesq buoyancy of the periodic solver (its step, nns_spec_ns_fields_buoyant_f32, nns_spec_ns_buoyancy_spectrum_f32)
def spec_ns_step_buoyant_(what, that, mean, ghat, work, ny, Lx, Ly, dt, nu, drag, kappa, grad, buoyancy, nsteps=1):
    """spec_ns_step_scalar_ with the scalar acting on the flow through buoyancy = (bx, by): w_t gains by theta_x - bx theta_y, every stage with
    its own theta^.  (0, 0) makes exactly the calls of spec_ns_step_scalar_.  No allocation, no host synchronisation: capturable."""
    return _spec_ns_step('nns_spec_ns_step_buoyant_f32', what, mean, work, ny, Lx, Ly, dt, (nu, drag, kappa, *grad, *buoyancy), nsteps,
                         that=that, ghat=ghat), that


# white-in-time stochastic forcing of the periodic solver
def _spec_ns_noise(who, amp, seed, clock, ids, B, my1, nx, device):
    """The checked noise arguments of a step: amp float32 [my1, nx], clock int64 [1] and ids int32 [B] on the state's device, seed a 64-bit int."""
    _spec_ns_f32(who, 'amp', amp, (my1, nx), device)
    for name, t, dtype, shape in (('clock', clock, torch.int64, (1,)), ('ids', ids, torch.int32, (B,))):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
            raise TypeError("%s: %s must be a contiguous %s device tensor" % (who, name, dtype))
        if tuple(t.shape) != shape:
            raise ValueError("%s: %s must be %s %s, got %s" % (who, name, dtype, list(shape), tuple(t.shape)))
    if clock.device != device or ids.device != device:
        raise ValueError("%s: clock and ids must be on the state's device %s" % (who, device))
    if isinstance(seed, bool) or not isinstance(seed, numbers.Integral):
        raise TypeError("%s: seed must be an int, got %r" % (who, seed))
    if not 0 <= seed < 2 ** 64:
        raise ValueError("%s: seed = %d must be in [0, 2^64)" % (who, seed))


def spec_ns_step_stochastic_(what, that, mean, ghat, work, ny, Lx, Ly, dt, nu, drag, kappa, grad, buoyancy, amp, seed, clock, ids, nsteps=1):
    """nsteps steps of spec_ns_step_buoyant_ (that None: of spec_ns_step_forced_; kappa, grad and buoyancy are then ignored), each followed by
    the kick w^ += sqrt(dt) amp xi(n, ids[b]): amp float32 [my1, nx] (shared by the batch), seed a 64-bit int, clock int64 [1] (the state's
    stochastic step count, advanced on the device) and ids int32 [B], all on the state's device.  No allocation, no host synchronisation:
    capturable, and a replay continues the noise sequence."""
    return _spec_ns_step('nns_spec_ns_step_stochastic_f32', what, mean, work, ny, Lx, Ly, dt, (nu, drag, kappa, *grad, *buoyancy), nsteps,
                         that=that, ghat=ghat, noise=(amp, seed, clock, ids), optional=('that',))


def spec_ns_fields_buoyant(what, that, mean, work, ny, Lx, Ly, rho, buoyancy, out=None):
    """(u, v, p) float32 [B, nx, ny] of a buoyant state: p also carries -rho i (k . b) theta^ / |k|^2.  work: spec_ns_scalar_workspace bytes;
    out as in spec_ns_fields."""
    B, my1, nx = _spec_ns_state('spec_ns_fields_buoyant', what, mean, work, ny)
    _spec_ns_same('spec_ns_fields_buoyant', that, what)
    u, v, p = out = _spec_ns_field_out('spec_ns_fields_buoyant', out, (B, nx, int(ny)), what.device)
    bx, by = buoyancy
    check(_lib.lib().nns_spec_ns_fields_buoyant_f32(_p(what), _p(that), _p(mean), _p(u), _p(v), _p(p), _p(work), work.numel(), B, nx, int(ny),
                                                    float(Lx), float(Ly), float(rho), float(bx), float(by), _stream()),
          'nns_spec_ns_fields_buoyant_f32')
    return out


def spec_ns_buoyancy_spectrum(what, that, ny, Lx, Ly, buoyancy, out=None):
    """float64 [B, nshell]: the buoyancy production <(b . u) theta'> per shell; its sum over the shells is b . (flux_x, flux_y) of
    spec_ns_scalar_diag."""
    B, my1, nx = _spec_ns_state('spec_ns_buoyancy_spectrum', what, None, None, ny)
    _spec_ns_same('spec_ns_buoyancy_spectrum', that, what)
    S = spec_ns_shells(nx, ny, Lx, Ly)[0]
    out = _spec_ns_out('spec_ns_buoyancy_spectrum', out, (B, S), what.device)
    bx, by = buoyancy
    check(_lib.lib().nns_spec_ns_buoyancy_spectrum_f32(_p(what), _p(that), _p(out), S, B, nx, int(ny), float(Lx), float(Ly), float(bx),
                                                       float(by), _stream()), 'nns_spec_ns_buoyancy_spectrum_f32')
    return out


# general linear operator of the periodic solver (its step, nns_spec_ns_linear_spectrum_f32)
def spec_ns_step_linear_(what, that, mean, ghat, work, ny, Lx, Ly, dt, kappa, grad, buoyancy, lin, amp=None, seed=0, clock=None, ids=None,
                         nsteps=1):
    """nsteps steps of spec_ns_step_stochastic_ (that None: no scalar; amp, clock and ids all None: no noise) with the vorticity's linear
    operator taken from lin, float32 [my1, nx, 2] = (Re, Im)(lambda dt / 2) on the state's device (shared by the batch), which holds viscosity
    and drag: neither is an argument.  No allocation, no host synchronisation: capturable."""
    return _spec_ns_step('nns_spec_ns_step_linear_f32', what, mean, work, ny, Lx, Ly, dt, (kappa, *grad, *buoyancy), nsteps, that=that,
                         ghat=ghat, lin=lin, noise=(amp, seed, clock, ids), optional=('that', 'noise'))


def spec_ns_advance_(what, that, mean, ghat, work, ny, Lx, Ly, dt, nu, drag, kappa, grad, buoyancy, lin=None, noise=None, nsteps=1):
    """nsteps steps by the least general of the six entries above that covers the arguments -- the one rule by which the package picks a
    step: a table lin: the linear step (nu and drag are then the table's); else noise = (amp, seed, clock, ids): the stochastic one; else a
    scalar that with buoyancy != (0, 0): the buoyant one; else a scalar: the scalar one; else a force ghat or drag > 0: the forced one; else
    the plain one."""
    box = (work, ny, Lx, Ly, dt)
    if lin is not None:
        return spec_ns_step_linear_(what, that, mean, ghat, *box, kappa, grad, buoyancy, lin, *(noise or (None, 0, None, None)), nsteps)
    if noise is not None:
        return spec_ns_step_stochastic_(what, that, mean, ghat, *box, nu, drag, kappa, grad, buoyancy, *noise, nsteps)
    if that is not None and tuple(buoyancy) != (0.0, 0.0):
        return spec_ns_step_buoyant_(what, that, mean, ghat, *box, nu, drag, kappa, grad, buoyancy, nsteps)[0]
    if that is not None:
        return spec_ns_step_scalar_(what, that, mean, ghat, *box, nu, drag, kappa, grad, nsteps)[0]
    if ghat is not None or drag > 0:
        return spec_ns_step_forced_(what, mean, ghat, *box, nu, drag, nsteps)
    return spec_ns_step_(what, mean, *box, nu, nsteps)


# forward mode of the periodic solver's step (nns_spec_ns_step_tangent_f32)
def spec_ns_tangent_workspace(B, nx, ny):
    """Bytes of the workspace spec_ns_step_tangent_ needs for B grids of nx x ny (>= spec_ns_workspace)."""
    return _query_bytes('nns_spec_ns_tangent_workspace', int(B), int(nx), int(ny))


def spec_ns_step_tangent_(what, dwhat, mean, ghat, dghat, work, ny, Lx, Ly, dt, nu, drag, lin=None, noise=None, nsteps=1):
    """nsteps steps of the flow and of a perturbation dwhat carried along with it, both in place: what bitwise as by spec_ns_advance_ with the
    same ghat, nu, drag, lin and noise = (amp, seed, clock, ids) (no scalar), dwhat <- J dwhat + (the response to) dghat, the Jacobian of
    those steps.  dwhat: float32 like what; dghat: the source's perturbation, float32 [1 or B, my1, nx, 2] or None; lin None: no table.
    work: spec_ns_tangent_workspace bytes.  8 launches per step and one per call, no allocation, no host synchronisation: capturable."""
    return _spec_ns_step('nns_spec_ns_step_tangent_f32', what, mean, work, ny, Lx, Ly, dt, (nu, drag), nsteps, dwhat=dwhat, ghat=ghat,
                         dghat=dghat, lin=lin, noise=noise, optional=('lin',)), dwhat


# forward mode of the scalar and the buoyant step (nns_spec_ns_step_scalar_tangent_f32)
def spec_ns_scalar_tangent_workspace(B, nx, ny):
    """Bytes of the workspace spec_ns_step_scalar_tangent_ needs for B grids of nx x ny (>= spec_ns_scalar_workspace and spec_ns_tangent_workspace)."""
    return _query_bytes('nns_spec_ns_scalar_tangent_workspace', int(B), int(nx), int(ny))


def spec_ns_step_scalar_tangent_(what, that, dwhat, dthat, mean, ghat, dghat, work, ny, Lx, Ly, dt, nu, drag, kappa, grad=(0.0, 0.0),
                                 buoyancy=(0.0, 0.0), lin=None, noise=None, nsteps=1):
    """nsteps steps of the system (what, that) and of a perturbation (dwhat, dthat) carried along with it, all four in place: (what, that)
    bitwise as by spec_ns_advance_ with the same arguments, (dwhat, dthat) <- J (dwhat, dthat) + (the response to) dghat, the Jacobian of
    those steps.  dwhat, dthat: float32 like what; dghat: the vorticity source's perturbation, float32 [1 or B, my1, nx, 2] or None.
    work: spec_ns_scalar_tangent_workspace bytes.  8 launches per step and one per call, no allocation, no host synchronisation: capturable."""
    (gx, gy), (bx, by) = grad, buoyancy
    _spec_ns_step('nns_spec_ns_step_scalar_tangent_f32', what, mean, work, ny, Lx, Ly, dt, (nu, drag, kappa, gx, gy, bx, by), nsteps, that=that,
                  dwhat=dwhat, dthat=dthat, ghat=ghat, dghat=dghat, lin=lin, noise=noise, optional=('lin',))
    return what, that, dwhat, dthat


# K tangents on one base and their orthonormalisation (nns_spec_ns_step_tangents_f32, nns_spec_ns_tangent_gram_f64, nns_spec_ns_tangent_combine_f32)
SPEC_NS_MAX_TANGENTS = 32


def spec_ns_tangents_workspace(B, K, nx, ny):
    """Bytes of the workspace spec_ns_step_tangents_ needs for K tangents on B grids of nx x ny (>= spec_ns_workspace)."""
    return _query_bytes('nns_spec_ns_tangents_workspace', int(B), int(K), int(nx), int(ny))


def _spec_ns_tangents(who, dwhat, ny, B=None, my1=None, nx=None, device=None):
    """(K, B, my1, nx) of the checked tangents dwhat, float32 [K, B, my1, nx, 2] with K in [1, 32]; B, my1, nx, device: those of the state
    they belong to (all None: the tangents alone, ny decides my1)."""
    _f32(dwhat)
    if dwhat.dim() != 5 or dwhat.shape[4] != 2:
        raise ValueError("%s: dwhat must be float32 [K, B, my1, nx, 2], got %s" % (who, tuple(dwhat.shape)))
    K = int(dwhat.shape[0])
    if not 1 <= K <= SPEC_NS_MAX_TANGENTS:
        raise ValueError("%s: K = %d tangents, must be in [1, %d]" % (who, K, SPEC_NS_MAX_TANGENTS))
    if B is None:
        B, my1, nx, device = int(dwhat.shape[1]), spec_ns_kept_y(ny), int(dwhat.shape[3]), dwhat.device
    if tuple(dwhat.shape[1:4]) != (B, my1, nx):
        raise ValueError("%s: dwhat must be float32 [K, %d, %d, %d, 2], got %s" % (who, B, my1, nx, tuple(dwhat.shape)))
    if dwhat.device != device:
        raise ValueError("%s: dwhat must be on the state's device %s" % (who, device))
    return K, B, my1, nx


def spec_ns_step_tangents_(what, dwhat, mean, ghat, work, ny, Lx, Ly, dt, nu, drag, lin=None, noise=None, nsteps=1):
    """spec_ns_step_tangent_ with K tangents dwhat (float32 [K, B, my1, nx, 2], K <= 32) on the one base what: what and every dwhat[k] bitwise
    as from that call with dwhat[k] alone (no dghat), the base's transforms done once for all K.  work: spec_ns_tangents_workspace bytes.
    8 launches per step and one per call, no allocation, no host synchronisation: capturable."""
    return _spec_ns_step('nns_spec_ns_step_tangents_f32', what, mean, work, ny, Lx, Ly, dt, (nu, drag), nsteps, dwhat=dwhat, members=True,
                         ghat=ghat, lin=lin, noise=noise, optional=('lin',)), dwhat


def spec_ns_tangent_gram(dwhat, ny, Lx, Ly, out=None):
    """float64 [B, K, K]: the energy inner products of the K tangents dwhat ([K, B, my1, nx, 2]) per grid, 1/2 <du_k . du_l>; the diagonal is
    spec_ns_diag's energy of each member.  Bitwise symmetric and repeatable.  No host synchronisation."""
    who = 'spec_ns_tangent_gram'
    K, B, my1, nx = _spec_ns_tangents(who, dwhat, ny)
    out = _spec_ns_out(who, out, (B, K, K), dwhat.device)
    check(_lib.lib().nns_spec_ns_tangent_gram_f64(_p(dwhat), K, _p(out), B, nx, int(ny), float(Lx), float(Ly), _stream()),
          'nns_spec_ns_tangent_gram_f64')
    return out


def spec_ns_tangent_combine_(dwhat, coef, ny):
    """dwhat[k] <- sum over l <= k of coef[b, l, k] dwhat[l] in place, coef float64 [B, K, K] upper triangular on dwhat's device: float64
    sums, rounded once.  No host synchronisation."""
    who = 'spec_ns_tangent_combine'
    K, B, my1, nx = _spec_ns_tangents(who, dwhat, ny)
    if not (isinstance(coef, torch.Tensor) and coef.is_cuda and coef.dtype == torch.float64 and coef.is_contiguous()):
        raise TypeError("%s: coef must be a contiguous float64 device tensor" % who)
    if tuple(coef.shape) != (B, K, K) or coef.device != dwhat.device:
        raise ValueError("%s: coef must be float64 [%d, %d, %d] on dwhat's device, got %s on %s" % (who, B, K, K, tuple(coef.shape), coef.device))
    check(_lib.lib().nns_spec_ns_tangent_combine_f32(_p(dwhat), K, _p(coef), B, nx, int(ny), _stream()), 'nns_spec_ns_tangent_combine_f32')
    return dwhat


# K tangent pairs on one base with a scalar (nns_spec_ns_step_scalar_tangents_f32, nns_spec_ns_tangent_variance_gram_f64)
def spec_ns_scalar_tangents_workspace(B, K, nx, ny):
    """Bytes of the workspace spec_ns_step_scalar_tangents_ needs for K tangent pairs on B grids of nx x ny (10 + 10 K compacted fields;
    K = 1 is spec_ns_scalar_tangent_workspace)."""
    return _query_bytes('nns_spec_ns_scalar_tangents_workspace', int(B), int(K), int(nx), int(ny))


def spec_ns_step_scalar_tangents_(what, that, dwhat, dthat, mean, ghat, work, ny, Lx, Ly, dt, nu, drag, kappa, grad=(0.0, 0.0),
                                  buoyancy=(0.0, 0.0), lin=None, noise=None, nsteps=1):
    """spec_ns_step_scalar_tangent_ with K pairs (dwhat, dthat) (float32 [K, B, my1, nx, 2] each, K <= 32) on the one base (what, that): the
    base and every pair (dwhat[k], dthat[k]) bitwise as from that call with the pair alone (no dghat), the base's transforms and column passes
    done once for all K.  work: spec_ns_scalar_tangents_workspace bytes.  8 launches per step and one per call, no allocation, no host
    synchronisation: capturable."""
    (gx, gy), (bx, by) = grad, buoyancy
    _spec_ns_step('nns_spec_ns_step_scalar_tangents_f32', what, mean, work, ny, Lx, Ly, dt, (nu, drag, kappa, gx, gy, bx, by), nsteps, that=that,
                  dwhat=dwhat, dthat=dthat, members=True, ghat=ghat, lin=lin, noise=noise, optional=('lin',))
    return what, that, dwhat, dthat


def spec_ns_tangent_variance_gram(dthat, ny, out=None):
    """float64 [B, K, K]: the variance inner products of the K scalar tangents dthat ([K, B, my1, nx, 2]) per grid, 1/2 <dtheta_k' dtheta_l'>
    (the means, the (0, 0) entries, do not enter); the diagonal is bitwise column 0 of spec_ns_scalar_diag of each member.  Bitwise
    symmetric and repeatable.  No host synchronisation."""
    who = 'spec_ns_tangent_variance_gram'
    K, B, my1, nx = _spec_ns_tangents(who, dthat, ny)
    out = _spec_ns_out(who, out, (B, K, K), dthat.device)
    check(_lib.lib().nns_spec_ns_tangent_variance_gram_f64(_p(dthat), K, _p(out), B, nx, int(ny), _stream()),
          'nns_spec_ns_tangent_variance_gram_f64')
    return out


def spec_ns_linear_spectrum(what, rate, ny, Lx, Ly, out=None):
    """float64 [B, 2, nshell]: (D_E, D_Z) per shell, the rates at which the linear term changes energy and enstrophy; rate = Re(lambda)
    float64 [my1, nx] on the state's device."""
    who = 'spec_ns_linear_spectrum'
    B, my1, nx = _spec_ns_state(who, what, None, None, ny)
    if not (isinstance(rate, torch.Tensor) and rate.is_cuda and rate.dtype == torch.float64 and rate.is_contiguous()):
        raise TypeError("%s: rate must be a contiguous float64 device tensor" % who)
    if tuple(rate.shape) != (my1, nx) or rate.device != what.device:
        raise ValueError("%s: rate must be float64 [%d, %d] on the state's device, got %s on %s" % (who, my1, nx, tuple(rate.shape), rate.device))
    S = spec_ns_shells(nx, ny, Lx, Ly)[0]
    out = _spec_ns_out(who, out, (B, 2, S), what.device)
    check(_lib.lib().nns_spec_ns_linear_spectrum_f32(_p(what), _p(rate), _p(out), S, B, nx, int(ny), float(Lx), float(Ly), _stream()),
          'nns_spec_ns_linear_spectrum_f32')
    return out


# ----------------------------------------------------------------------------- physics-informed loss head
_PINN_WS = {}


def _pinn_ws(device):
    """The head's workspace (per-block partial sums + the arrival counter), zeroed once per device and stream."""
    key = (device, _stream())
    if key not in _PINN_WS:
        _PINN_WS[key] = torch.zeros(int(_lib.lib().nns_pinn_workspace_bytes()) // 8 + 1, dtype=torch.float64, device=device)
    return _PINN_WS[key]


class PinnHeadFn(torch.autograd.Function):
    """total, data, phys = head(mlp_out, state, target): pred = state + mlp_out, data = mean (pred - target)^2, phys = mean-square residual of pred,
    total = data + lam phys (nns/neural_spectral/physics_informed.py) as ONE autograd node: nns_pinn_assemble_f32 -> the residual kernel ->
    nns_pinn_loss_f32 forward; the residual adjoint -> nns_pinn_combine_f32 backward.  mlp_out, state, target: contiguous float32 [batch, 3, ...]
    (channel-major fields: batch = 1); `residual` = (kind, consts): ('fd', (dt, dx, dy, rho, nu, stencil)) or ('spectral', (dt, Lx, Ly, rho, nu, precise));
    dims = the fields' (B, nx, ny)."""

    @staticmethod
    def forward(ctx, out, state, target, residual, dims, lam, w_div):
        for t in (out, state) + ((target,) if target is not None else ()):
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape == out.shape):
                raise ValueError("PinnHeadFn: mlp_out, state and target must be contiguous float32 device tensors of one shape")
        B, nx, ny = dims
        batch, npix = out.shape[0], out[0, 0].numel()
        if out.shape[1] != 3 or batch * npix != B * nx * ny:
            raise ValueError("PinnHeadFn: fields [batch, 3, ...] with batch x pixels = %d x %d x %d expected, got %s" % (B, nx, ny, tuple(out.shape)))
        L, st, ws = _lib.lib(), _stream(), _pinn_ws(out.device)
        new = lambda: torch.empty((B, nx, ny), dtype=torch.float32, device=out.device)
        u, v, p = new(), new(), new()
        if batch == 1:                                   # channel-major: the state's channels ARE contiguous fields
            u_prev, v_prev, pu, pv = state[0, 0].reshape(B, nx, ny), state[0, 1].reshape(B, nx, ny), None, None
        else:
            u_prev, v_prev = new(), new()
            pu, pv = _p(u_prev), _p(v_prev)
        check(L.nns_pinn_assemble_f32(_p(out), _p(state), _p(target) if target is not None else None, _p(u), _p(v), _p(p), pu, pv, _p(ws),
                                      batch, npix, st), 'nns_pinn_assemble_f32')
        kind, c = residual
        if kind == 'fd':
            r = fd_residual(u, v, p, u_prev, v_prev, *c)
        else:
            r = spec_residual(u, v, p, u_prev, v_prev, *c)
        out3 = torch.empty(3, dtype=torch.float32, device=out.device)
        n = B * nx * ny
        n_data = 3.0 * n if target is not None else 0.0
        check(L.nns_pinn_loss_f32(_p(r[0]), _p(r[1]), _p(r[2]), n, _p(ws), n_data, float(lam), float(w_div), _p(out3), st), 'nns_pinn_loss_f32')
        ctx.save_for_backward(u, v, p, r[0], r[1], r[2], target)
        ctx.consts = (residual, (B, nx, ny), batch, npix, float(lam), n, n_data, out.shape)
        ctx.set_materialize_grads(False)
        return out3.unbind(0)                            # total, data, phys

    @staticmethod
    def backward(ctx, g_total, g_data, g_phys):
        u, v, p, ru, rv, rd, target = ctx.saved_tensors
        residual, (B, nx, ny), batch, npix, lam, n, n_data, shape = ctx.consts
        kind, c = residual
        if kind == 'fd':
            gu, gv, gp, _, _ = fd_residual_bwd(u, v, ru, rv, rd, *c, want_prev=False)
        else:
            gu, gv, gp, _, _ = spec_residual_bwd(u, v, ru, rv, rd, *c, want_prev=False)
        zero = lambda g: torch.zeros((), dtype=torch.float32, device=u.device) if g is None else g.to(torch.float32)
        if g_data is None and g_phys is None:            # the training step: total.backward()
            up_d = up_p = zero(g_total).contiguous()
            c_phys = 2.0 * lam / n
        else:                                            # someone differentiates the parts: d/d data = g_total + g_data, d/d phys = lam g_total + g_phys
            up_d = (zero(g_total) + zero(g_data)).contiguous()
            up_p = (lam * zero(g_total) + zero(g_phys)).contiguous()
            c_phys = 2.0 / n
        grad = torch.empty(shape, dtype=torch.float32, device=u.device)
        check(_lib.lib().nns_pinn_combine_f32(_p(gu), _p(gv), _p(gp), _p(u), _p(v), _p(p), _p(target) if target is not None else None,
                                              _p(up_d), _p(up_p), 2.0 / n_data if n_data else 0.0, c_phys, _p(grad), batch, npix, _stream()),
              'nns_pinn_combine_f32')
        return grad, None, None, None, None, None, None


# reverse mode of the periodic solver's forced step
def spec_ns_adjoint_workspace(B, nx, ny):
    """Bytes of the workspace spec_ns_step_adjoint_ needs for B grids of nx x ny (>= spec_ns_workspace)."""
    return _query_bytes('nns_spec_ns_adjoint_workspace', int(B), int(nx), int(ny))


def _spec_ns_adjoint_tensors(who, lam, ghat, gbar, **starts):
    """gbatch of an adjoint call after the checks of its start spectra (what0, that0: [nsteps] + lam's shape, equal nsteps), ghat and gbar."""
    nsteps = None
    for name, t in starts.items():
        _f32(t)
        nsteps = t.shape[0] if nsteps is None and t.dim() else nsteps
        if t.dim() != 5 or tuple(t.shape[1:]) != tuple(lam.shape) or t.device != lam.device or t.shape[0] != nsteps:
            raise ValueError("%s: %s must be float32 [nsteps, %d, %d, %d, 2] on the state's device, got %s"
                             % ((who, name) + tuple(lam.shape[:3]) + (tuple(t.shape),)))
    gbatch = _spec_ns_force(who, ghat, lam)
    if gbar is not None:
        _spec_ns_same(who, gbar, lam, 'gbar')
    return gbatch


def _spec_ns_adjoint(entry, what0, mean, ghat, lam, gbar, work, ny, Lx, Ly, dt, numbers, scalar=_ABSENT, optional=False, lin=_ABSENT,
                     lbar=_ABSENT):
    """Every adjoint call: the checks of the tensors, then the call of `entry`, whose arguments are what0, [that0,] mean, ghat, gbatch, lam,
    [mu,] gbar, work, its size, the box and dt, `numbers` (the entry's doubles after dt), [lin,] nsteps (what0's) and the stream [, lbar].
    scalar = (that0, mu), lin, lbar: the bracketed ones the entry has; `optional`: it takes that0 and mu as NULL (both None: no scalar).  The
    caller's name in the messages is the entry's without nns_ and f32."""
    who = entry[4:-3]
    B, my1, nx = _spec_ns_state(who, lam, mean, work, ny)
    that0, mu = (None, None) if scalar is _ABSENT else scalar
    if optional and (that0 is None) != (mu is None):
        raise ValueError("%s: that0 and mu must be both None (no scalar) or both given" % who)
    starts = {'what0': what0}
    if scalar is not _ABSENT and not (optional and that0 is None):
        _spec_ns_same(who, mu, lam, 'mu')
        starts['that0'] = that0
    gbatch = _spec_ns_adjoint_tensors(who, lam, ghat, gbar, **starts)
    args = [_p(what0)]
    if scalar is not _ABSENT:
        args.append(_pn(that0))
    args += (_p(mean), _pn(ghat), gbatch, _p(lam))
    if scalar is not _ABSENT:
        args.append(_pn(mu))
    args += (_pn(gbar), _p(work), work.numel(), B, nx, int(ny), float(Lx), float(Ly), float(dt))
    args.extend(map(float, numbers))
    if lin is not _ABSENT:
        _spec_ns_f32(who, 'lin', lin, (my1, nx, 2), lam.device)
        args.append(_p(lin))
    args += (int(what0.shape[0]), _stream())
    if lbar is not _ABSENT:
        if lbar is not None:
            _spec_ns_same(who, lbar, lam, 'lbar')
        args.append(_pn(lbar))
    check(getattr(_lib.lib(), entry)(*args), entry)


def spec_ns_step_adjoint_(what0, mean, ghat, lam, gbar, work, ny, Lx, Ly, dt, nu, drag):
    """The vector-Jacobian product of the nsteps forced steps whose start spectra are what0 (float32 [nsteps, B, my1, nx, 2], only read): lam
    ([B, my1, nx, 2]) holds, in, the cotangent of the state after the last step and, out, that of the state before the first; gbar (the same
    shape, or None) receives the cotangent of g^, one per grid, summed over the steps.  mean, ghat, dt, nu, drag: the forward's.  Cotangents
    are spectra of real fields paired by the grid sum.  work: spec_ns_adjoint_workspace bytes.  16 launches per step, no allocation, no host
    synchronisation."""
    _spec_ns_adjoint('nns_spec_ns_step_adjoint_f32', what0, mean, ghat, lam, gbar, work, ny, Lx, Ly, dt, (nu, drag))
    return lam, gbar


# reverse mode of the periodic solver's scalar and buoyant step
def spec_ns_scalar_adjoint_workspace(B, nx, ny):
    """Bytes of the workspace spec_ns_step_scalar_adjoint_ needs for B grids of nx x ny (>= every other spec_ns workspace)."""
    return _query_bytes('nns_spec_ns_scalar_adjoint_workspace', int(B), int(nx), int(ny))


def spec_ns_step_scalar_adjoint_(what0, that0, mean, ghat, lam, mu, gbar, work, ny, Lx, Ly, dt, nu, drag, kappa, grad=(0.0, 0.0),
                                 buoyancy=(0.0, 0.0)):
    """spec_ns_step_adjoint_ for the system (w^, theta^) of spec_ns_step_scalar_ / spec_ns_step_buoyant_: what0, that0 (float32
    [nsteps, B, my1, nx, 2], only read) are the spectra at the start of every step; lam and mu ([B, my1, nx, 2]) hold, in, the cotangents of
    (w^, theta^) after the last step and, out, those of the pair before the first; gbar (the same shape, or None) receives the cotangent of the
    vorticity source g^, one per grid, summed over the steps.  mean, ghat, dt, nu, drag, kappa, grad, buoyancy: the forward's (buoyancy
    (0, 0): the passive scalar).  work: spec_ns_scalar_adjoint_workspace bytes.  16 launches per step, no allocation, no host synchronisation."""
    _spec_ns_adjoint('nns_spec_ns_step_scalar_adjoint_f32', what0, mean, ghat, lam, gbar, work, ny, Lx, Ly, dt,
                     (nu, drag, kappa, *grad, *buoyancy), scalar=(that0, mu))
    return lam, mu, gbar


# reverse mode of the periodic solver's linear step, with or without its scalar, buoyancy and noise
def spec_ns_step_linear_adjoint_(what0, that0, mean, ghat, lam, mu, gbar, work, ny, Lx, Ly, dt, kappa, grad, buoyancy, lin):
    """spec_ns_step_adjoint_ (that0 and mu None; kappa, grad and buoyancy are then ignored; work: spec_ns_adjoint_workspace bytes) or
    spec_ns_step_scalar_adjoint_ (both given; work: spec_ns_scalar_adjoint_workspace bytes) for the steps of spec_ns_step_linear_: the
    vorticity's factors are the conjugates of the forward's, from the same table lin, float32 [my1, nx, 2] = (Re, Im)(lambda dt / 2) on the
    state's device, which holds viscosity and drag: neither is an argument.  A stochastic step's adjoint is this call on the start spectra the
    noisy forward saved: the kick's Jacobian is the identity.  16 launches per step, no allocation, no host synchronisation."""
    _spec_ns_adjoint('nns_spec_ns_step_linear_adjoint_f32', what0, mean, ghat, lam, gbar, work, ny, Lx, Ly, dt, (kappa, *grad, *buoyancy),
                     scalar=(that0, mu), optional=True, lin=lin)
    return lam, mu, gbar


# the same reverse mode, also differentiated in the linear operator's table
def spec_ns_step_operator_adjoint_(what0, that0, mean, ghat, lam, mu, gbar, work, ny, Lx, Ly, dt, kappa, grad, buoyancy, lin, lbar):
    """spec_ns_step_linear_adjoint_ whose launches also sum the cotangent of the table lin into lbar (float32 [B, my1, nx, 2] on the state's
    device, overwritten): one per grid, summed over the steps of the call, zero off the band and at (0, 0), BEFORE the weight of the cotangent
    convention -- include/nns.h gives the table gradient it stands for (PeriodicSolver.evolve applies it).  lbar None: exactly
    spec_ns_step_linear_adjoint_.  The same 16 launches per step, no allocation, no host synchronisation."""
    _spec_ns_adjoint('nns_spec_ns_step_operator_adjoint_f32', what0, mean, ghat, lam, gbar, work, ny, Lx, Ly, dt, (kappa, *grad, *buoyancy),
                     scalar=(that0, mu), optional=True, lin=lin, lbar=lbar)
    return lam, mu, gbar, lbar


def spec_ns_adjoint_(what0, that0, mean, ghat, lam, mu, gbar, work, ny, Lx, Ly, dt, nu, drag, kappa, grad, buoyancy, lin=None, lbar=None):
    """The adjoint of the steps spec_ns_advance_ takes, by the least general of the four entries above that covers the arguments -- the one
    rule by which the package picks an adjoint: lbar: the operator's (needs lin); else a table lin: the linear one; else a scalar (that0 and
    mu): the scalar one; else the flow's.  Noise changes nothing: the kick's Jacobian is the identity.  Returns (lam, mu, gbar, lbar)."""
    box = (work, ny, Lx, Ly, dt)
    if lbar is not None:
        spec_ns_step_operator_adjoint_(what0, that0, mean, ghat, lam, mu, gbar, *box, kappa, grad, buoyancy, lin, lbar)
    elif lin is not None:
        spec_ns_step_linear_adjoint_(what0, that0, mean, ghat, lam, mu, gbar, *box, kappa, grad, buoyancy, lin)
    elif that0 is not None:
        spec_ns_step_scalar_adjoint_(what0, that0, mean, ghat, lam, mu, gbar, *box, nu, drag, kappa, grad, buoyancy)
    else:
        spec_ns_step_adjoint_(what0, mean, ghat, lam, gbar, *box, nu, drag)
    return lam, mu, gbar, lbar


# second-order adjoint of the periodic solver's flow step (nns_spec_ns_step_second_adjoint_f32)
def spec_ns_second_adjoint_workspace(B, nx, ny):
    """Bytes of the workspace spec_ns_second_adjoint_ needs for B grids of nx x ny (>= spec_ns_adjoint_workspace and spec_ns_tangent_workspace)."""
    return _query_bytes('nns_spec_ns_second_adjoint_workspace', int(B), int(nx), int(ny))


def spec_ns_second_adjoint_(what0, dwhat0, mean, ghat, dghat, lam, dlam, gbar, dgbar, work, ny, Lx, Ly, dt, nu, drag, lin=None):
    """spec_ns_step_adjoint_ (lin None) or spec_ns_step_linear_adjoint_ without a scalar (lin: the forward's table; nu and drag are then
    ignored) together with its derivative in a direction: what0, dwhat0 (float32 [nsteps, B, my1, nx, 2], only read) are the spectrum and its
    tangent at the start of every step of a spec_ns_step_tangent_ forward, dghat the source's perturbation of that forward ([1 or B, my1, nx, 2]
    or None); lam and dlam ([B, my1, nx, 2]) hold, in, the cotangent of the state after the last step and its derivative and, out, (wbar, dwbar)
    before the first; gbar and dgbar (the same shape, each or both None) receive the cotangent of g^ and its derivative, one per grid, summed
    over the steps.  lam and gbar are bitwise the first-order call's.  work: spec_ns_second_adjoint_workspace bytes.  16 launches per step, no
    allocation, no host synchronisation."""
    who = 'spec_ns_step_second_adjoint'
    B, my1, nx = _spec_ns_state(who, lam, mean, work, ny)
    _spec_ns_same(who, dlam, lam, 'dlam')
    gbatch = _spec_ns_adjoint_tensors(who, lam, ghat, gbar, what0=what0, dwhat0=dwhat0)
    dgbatch = _spec_ns_force(who, dghat, lam)
    if dgbar is not None:
        _spec_ns_same(who, dgbar, lam, 'dgbar')
    if lin is not None:
        _spec_ns_f32(who, 'lin', lin, (my1, nx, 2), lam.device)
    check(_lib.lib().nns_spec_ns_step_second_adjoint_f32(_p(what0), _p(dwhat0), _p(mean), _pn(ghat), gbatch, _pn(dghat), dgbatch, _p(lam), _p(dlam),
                                                         _pn(gbar), _pn(dgbar), _p(work), work.numel(), B, nx, int(ny), float(Lx), float(Ly),
                                                         float(dt), float(nu), float(drag), _pn(lin), int(what0.shape[0]), _stream()),
          'nns_spec_ns_step_second_adjoint_f32')
    return lam, dlam, gbar, dgbar


# Lagrangian tracers of the periodic solver (nns_spec_ns_particle_*)
PARTICLE_FIELDS = ('u', 'v', 'w', 'theta')           # bit k of a field mask names PARTICLE_FIELDS[k]


def spec_ns_particle_workspace(B, nfields, nx, ny):
    """Bytes of the workspace spec_ns_particle_coefs needs for nfields fields of B grids of nx x ny."""
    return _query_bytes('nns_spec_ns_particle_workspace', int(B), int(nfields), int(nx), int(ny))


def _spec_ns_f64(who, name, t, shape, device):
    """t is a contiguous float64 tensor of `shape` on the state's device."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()):
        raise TypeError("%s: %s must be a contiguous float64 device tensor" % (who, name))
    if tuple(t.shape) != tuple(shape) or t.device != device:
        raise ValueError("%s: %s must be float64 %s on %s, got %s on %s" % (who, name, list(shape), device, tuple(t.shape), t.device))


def spec_ns_particle_coefs(what, that, mean, coef, fields, order, work, ny, Lx, Ly):
    """coef (float32 [nfields, B, nx, ny]) <- the order-4 or order-6 B-spline coefficients of the fields of the mask `fields` (bit 0 u, 1 v,
    2 w, 3 theta, stored by ascending bit) of the state (what, mean[, that]).  work: spec_ns_particle_workspace bytes.  One launch and an
    inverse transform, no allocation, no host synchronisation."""
    who = 'spec_ns_particle_coefs'
    B, my1, nx = _spec_ns_state(who, what, mean, work, ny)
    if that is not None:
        _spec_ns_same(who, that, what)
    fields = int(fields)
    _spec_ns_f32(who, 'coef', coef, (bin(fields & 15).count('1'), B, nx, int(ny)), what.device)
    check(_lib.lib().nns_spec_ns_particle_coefs_f32(_p(what), _pn(that), _p(mean), _p(coef), fields, int(order), _p(work), work.numel(), B, nx,
                                                    int(ny), float(Lx), float(Ly), _stream()), 'nns_spec_ns_particle_coefs_f32')
    return coef


def _spec_ns_particle_coef(who, coef, nfields=None):
    """(nfields, B, nx, ny) of the checked coefficient images."""
    _f32(coef)
    if coef.dim() != 4 or (nfields is not None and coef.shape[0] != nfields):
        raise ValueError("%s: coef must be float32 [%s, B, nx, ny], got %s" % (who, 'nfields' if nfields is None else nfields, tuple(coef.shape)))
    return tuple(coef.shape)


def spec_ns_particle_sample(coef, pos, order, Lx, Ly, out=None):
    """float32 [B, P, nfields]: the splines of the coefficient images coef [nfields, B, nx, ny] at the positions pos (float64 [B, P, 2])."""
    who = 'spec_ns_particle_sample'
    nf, B, nx, ny = _spec_ns_particle_coef(who, coef)
    if not (isinstance(pos, torch.Tensor) and pos.dim() == 3):
        raise ValueError("%s: pos must be float64 [B, P, 2]" % who)
    P = pos.shape[1]
    _spec_ns_f64(who, 'pos', pos, (B, P, 2), coef.device)
    if out is None:
        out = torch.empty((B, P, nf), dtype=torch.float32, device=coef.device)
    else:
        _spec_ns_f32(who, 'out', out, (B, P, nf), coef.device)
    check(_lib.lib().nns_spec_ns_particle_sample_f32(_p(coef), _p(pos), _p(out), nf, int(order), B, P, nx, ny, float(Lx), float(Ly), _stream()),
          'nns_spec_ns_particle_sample_f32')
    return out


def spec_ns_particle_stage_(coef, pos0, pos_in, pos_out, acc, a, wk, c, first, closing, order, Lx, Ly):
    """One Runge-Kutta stage on the images coef = (u, v) [2, B, nx, ny]: k = (u, v)(pos_in); s = (0 if first else acc) + wk k; closing:
    pos_out <- pos0 + c s; else acc <- s and pos_out <- pos0 + a k.  All positions and acc float64 [B, P, 2] (include/nns.h names the
    aliasing allowed).  One launch, no allocation, no host synchronisation."""
    who = 'spec_ns_particle_stage'
    nf, B, nx, ny = _spec_ns_particle_coef(who, coef, 2)
    if not (isinstance(pos0, torch.Tensor) and pos0.dim() == 3):
        raise ValueError("%s: pos0 must be float64 [B, P, 2]" % who)
    shape = (B, pos0.shape[1], 2)
    for name, t in (('pos0', pos0), ('pos_in', pos_in), ('pos_out', pos_out)) + ((('acc', acc),) if acc is not None else ()):
        _spec_ns_f64(who, name, t, shape, coef.device)
    check(_lib.lib().nns_spec_ns_particle_stage_f32(_p(coef), _p(pos0), _p(pos_in), _p(pos_out), _pn(acc), float(a), float(wk), float(c),
                                                    int(bool(first)), int(bool(closing)), int(order), B, shape[1], nx, ny, float(Lx), float(Ly),
                                                    _stream()), 'nns_spec_ns_particle_stage_f32')
    return pos_out


# reverse mode of the sampling (nns_spec_ns_particle_cells_i32, _spread_f32, _sample_grad_f32, _coefs_adjoint_f32)
def _spec_ns_particle_pos(who, pos, B, device):
    """P of the checked positions, float64 [B, P, 2]."""
    if not (isinstance(pos, torch.Tensor) and pos.dim() == 3):
        raise ValueError("%s: pos must be float64 [B, P, 2]" % who)
    _spec_ns_f64(who, 'pos', pos, (B, pos.shape[1], 2), device)
    return pos.shape[1]


def spec_ns_particle_cells(pos, nx, ny, Lx, Ly):
    """(perm, start) of the positions pos (float64 [B, P, 2]) on B grids of nx x ny: perm, int64 [B P], the particle (an index into [B, P])
    of every slot of the order sorted by cell (b nx + ci) ny + cj, the particles of one cell in ascending index; start, int32
    [B nx ny + 1], the first slot of every cell, then B P.  One launch, then torch.sort(stable=True) and torch.searchsorted on the device:
    no host synchronisation."""
    who = 'spec_ns_particle_cells'
    B = pos.shape[0] if isinstance(pos, torch.Tensor) and pos.dim() == 3 else None
    P = _spec_ns_particle_pos(who, pos, B, getattr(pos, 'device', None))
    key = torch.empty(B * P, dtype=torch.int32, device=pos.device)
    check(_lib.lib().nns_spec_ns_particle_cells_i32(_p(pos), _p(key), B, P, int(nx), int(ny), float(Lx), float(Ly), _stream()),
          'nns_spec_ns_particle_cells_i32')
    key, perm = torch.sort(key, stable=True)
    cells = torch.arange(B * int(nx) * int(ny) + 1, dtype=torch.int32, device=pos.device)
    return perm, torch.searchsorted(key, cells, out_int32=True)


def spec_ns_particle_spread_workspace(B, P, order):
    """Bytes of the workspace spec_ns_particle_spread needs: one record of 2 order + 4 floats per particle."""
    return _query_bytes('nns_spec_ns_particle_spread_workspace', int(B), int(P), int(order))


def spec_ns_particle_spread(cot, pos, perm, start, nx, ny, order, Lx, Ly, out=None, work=None):
    """float32 [nfields, B, nx, ny]: the transpose of spec_ns_particle_sample applied to cot (float32 [B, P, nfields]); (perm, start) from
    spec_ns_particle_cells of pos.  Two launches, no atomics: repeats bitwise; every node is written."""
    who = 'spec_ns_particle_spread'
    _f32(cot)
    if cot.dim() != 3 or not 1 <= cot.shape[2] <= 4:
        raise ValueError("%s: cot must be float32 [B, P, nfields] with nfields in [1, 4], got %s" % (who, tuple(cot.shape)))
    B, P, nf = cot.shape
    nx, ny = int(nx), int(ny)
    if _spec_ns_particle_pos(who, pos, B, cot.device) != P:
        raise ValueError("%s: pos is for %d particles, cot for %d" % (who, pos.shape[1], P))
    for name, t, dtype, n in (('perm', perm, torch.int64, B * P), ('start', start, torch.int32, B * nx * ny + 1)):
        if not (isinstance(t, torch.Tensor) and t.dtype == dtype and t.is_contiguous() and t.device == cot.device and tuple(t.shape) == (n,)):
            raise ValueError("%s: %s must be a contiguous %s tensor [%d] on %s (from spec_ns_particle_cells)" % (who, name, dtype, n, cot.device))
    if out is None:
        out = torch.empty((nf, B, nx, ny), dtype=torch.float32, device=cot.device)
    else:
        _spec_ns_f32(who, 'out', out, (nf, B, nx, ny), cot.device)
    if work is None:
        work = torch.empty(spec_ns_particle_spread_workspace(B, P, order), dtype=torch.uint8, device=cot.device)
    check(_lib.lib().nns_spec_ns_particle_spread_f32(_p(cot), _p(pos), _p(perm), _p(start), _p(out), nf, int(order), _p(work), work.numel(), B, P,
                                                     nx, ny, float(Lx), float(Ly), _stream()), 'nns_spec_ns_particle_spread_f32')
    return out


def spec_ns_particle_sample_grad(coef, pos, order, Lx, Ly, out=None):
    """float32 [B, P, nfields, 2]: (d/dx, d/dy) of the splines of the coefficient images coef [nfields, B, nx, ny] at pos (float64 [B, P, 2])."""
    who = 'spec_ns_particle_sample_grad'
    nf, B, nx, ny = _spec_ns_particle_coef(who, coef)
    P = _spec_ns_particle_pos(who, pos, B, coef.device)
    if out is None:
        out = torch.empty((B, P, nf, 2), dtype=torch.float32, device=coef.device)
    else:
        _spec_ns_f32(who, 'out', out, (B, P, nf, 2), coef.device)
    check(_lib.lib().nns_spec_ns_particle_sample_grad_f32(_p(coef), _p(pos), _p(out), nf, int(order), B, P, nx, ny, float(Lx), float(Ly),
                                                          _stream()), 'nns_spec_ns_particle_sample_grad_f32')
    return out


def spec_ns_particle_coefs_adjoint(cbar, fields, order, Lx, Ly, work=None):
    """(wbar_hat, thbar_hat), float32 [B, my1, nx, 2] each (None where the mask `fields` has none of bits 0-2 / no bit 3): the transpose of
    spec_ns_particle_coefs applied to the cotangents cbar (float32 [nfields, B, nx, ny], by ascending bit).  work:
    spec_ns_particle_workspace bytes.  One forward transform and one pointwise launch."""
    who = 'spec_ns_particle_coefs_adjoint'
    nf, B, nx, ny = _spec_ns_particle_coef(who, cbar)
    fields = int(fields)
    if nf != bin(fields & 15).count('1'):
        raise ValueError("%s: cbar holds %d images, the mask %d names %d" % (who, nf, fields, bin(fields & 15).count('1')))
    shape = (B, spec_ns_kept_y(ny), nx, 2)
    wbar = torch.empty(shape, dtype=torch.float32, device=cbar.device) if fields & 7 else None
    thbar = torch.empty(shape, dtype=torch.float32, device=cbar.device) if fields & 8 else None
    if work is None:
        work = torch.empty(spec_ns_particle_workspace(B, nf, nx, ny), dtype=torch.uint8, device=cbar.device)
    check(_lib.lib().nns_spec_ns_particle_coefs_adjoint_f32(_p(cbar), _pn(wbar), _pn(thbar), fields, int(order), _p(work), work.numel(), B, nx, ny,
                                                            float(Lx), float(Ly), _stream()), 'nns_spec_ns_particle_coefs_adjoint_f32')
    return wbar, thbar
