// Pseudo-spectral 2-D Navier-Stokes on the periodic box [0, Lx) x [0, Ly), vorticity-streamfunction form, gfx950
// (include/nns.h: nns_spec_ns_*; restatement: tests/pspec_oracle.py).
//
// State: the vorticity spectrum w^ (numpy.fft.rfft2 convention, unnormalised) of every grid, kept COMPACTED and TRANSPOSED:
// only the kept y-wavenumbers j < my1 = (ny - 1) / 3 + 1 (the 2/3 rule, 3 j < ny) are stored, as complex lines along x,
// W[b][j][i] (i = x-wavenumber index, fftfreq order), plus the conserved mean velocity (U0, V0) per grid.
//
// Time step: integrating-factor (Lawson) RK4 with L = -nu |k|^2; each of the four stages is TWO launches:
//   ps_row_kernel<ny>   one line per grid row i (B nx lines): the c2r of (u, v, w_x, w_y) along y from their kept
//                       y-wavenumbers (two complex inverse transforms, u + i v and w_x + i w_y: Hermitian packing), the
//                       product u w_x + v w_y in registers, its r2c, and the kept part j < my1 written to Ph[b][i][j].
//   ps_col_kernel<nx,S> one line per kept column (b, j) (B my1 lines): Ph's column through an LDS transpose, the forward
//                       transform along x, N^ = -M P^, the Lawson update of stage S of W and the accumulator A (lane-owned,
//                       coalesced), then the next stage's four spectra i ky psi^, -i kx psi^, i kx w^, i ky w^ (scaled by
//                       1 / (nx ny), the means put in the (0, 0) mode) inverse-transformed along x and written, through the same
//                       LDS transpose, to G[f][b][i][j].
// Stage 4 of step n also prepares stage 1 of step n + 1 (w^ is the next stage input); a call starts with one column launch
// (S = 0) that only prepares.  Nothing but the kept third of the spectral columns is ever read, transformed or written.
// Decay factors are applied as z + expm1(x) z: the float32 rounding of E itself would be a systematic per-step error.
//
// Forcing and drag (nns_spec_ns_step_forced_f32; restatement: tests/pspec_forced_oracle.py): w_t + u w_x + v w_y = nu lap w - alpha w + g.
// ps_col_kernel<nx, S, FORCED = true> adds the constant g^ (the state's layout, one per grid or one shared by the batch) to N^ in every
// stage and uses L = -(nu |k|^2 + alpha); FORCED = false is the unforced code, argument list included.  ps_diag_kernel: energy,
// enstrophy and power input per grid from w^ (and g^) by Parseval.
//
// Passive scalar (nns_spec_ns_step_scalar_f32; restatement: tests/pspec_scalar_oracle.py): theta_t + u theta_x + v theta_y = kappa lap theta
// - (Gx u + Gy v), theta^ = M_theta rfft2(theta) in the layout of W with the (0, 0) mode KEPT (the mean of theta is state), integrated with w^
// as one system by the same Lawson RK4 (L_theta = -kappa |k|^2: no drag).  SCALAR = true rides in the same launches: the row pass
// inverse-transforms theta_x + i theta_y as well, forms u (theta_x + Gx) + v (theta_y + Gy) from the u, v it holds in registers and writes its
// kept modes to a second Ph field; the column pass, after the vorticity's work on a tile, stages that field, updates theta^ and its
// accumulator and prepares i kx theta^, i ky theta^ as G fields 4 and 5.  The vorticity's arithmetic is the unscalared kernel's, so w^ is
// bitwise what it is without a scalar; SCALAR = false is the present code, argument list included.
//
// Buoyancy (nns_spec_ns_step_buoyant_f32; restatement: tests/pspec_buoyant_oracle.py): the scalar acts on the flow through b theta', which adds
// by theta_x - bx theta_y to the vorticity equation, N^ += M (i kx by - i ky bx) theta^ with every stage's own theta^.  BUOYANT = true (SCALAR only) is
// the row pass's: the kept y-modes of theta_x and theta_y of a row ARE G fields 4 and 5 of that row (x-physical, y-spectral, scaled by 1 / (nx ny)),
// and the combination is linear, so -ny (by G4 - bx G5) is added to the forward-transformed product just before it is stored to Ph (ny: an
// unnormalised inverse then forward transform along y).  No further transform, no further line live across one; the column pass is untouched.
// b = 0 launches the passive kernels.  ps_pressure_buoyant_kernel adds -rho i (k . b) theta^ / |k|^2 to p^ (div (b theta') != 0).
//
// Stochastic forcing (nns_spec_ns_step_stochastic_f32; restatement: tests/pspec_stochastic_oracle.py): after the complete deterministic step the
// vorticity spectrum gets one white-in-time kick, w^ += sqrt(dt) a_k xi_k(n, id_b) on the kept modes, a the amplitude table [my1][nx] shared by
// the batch and xi a complex standard normal (E |xi|^2 = 1) from Philox4x32-10 keyed by the seed and counted by (step n, stored mode, grid id).
// A trailing PsStoch in the column kernel's argument pack (STOCH) is the compile-time switch, and only stages 1 and 4 have that form: stage 4
// evaluates the generator in registers where a_k != 0, just before w^ is stored and handed to the next step's stage 1; stage 1 advances the
// device-side step count (one lane of one workgroup: nothing in that launch reads it), so stage 4 reads n = clock - 1 and a captured step
// replays.  No further launch, transform or stream; kernels without the PsStoch keep their names and their code.
//
// General linear operator (nns_spec_ns_step_linear_f32; restatement: tests/pspec_linear_oracle.py): hyperviscosity, hypofriction and the beta
// effect are diagonal in Fourier space, so they only change the Lawson factor: lambda_k = -(nu |k|^2 + drag + nu_h |k|^2p + mu |k|^-2q)
// + i beta kx / |k|^2 comes as the float32 table lin = lambda dt / 2 [my1][nx][2], shared by the batch.  A PsLinear in the column kernel's
// argument pack (LINEAR) is the compile-time switch, and only stages 1-3 have that form (stage 4 applies no factor: a linear step ends in the
// forced or the stochastic stage-4 kernel).  There the vorticity's E - 1 and E^2 - 1 are complex: one 8-byte load per mode where the real form
// computes |k|^2, then one expm1 and one sincospi of the half angle where it has two expm1 (ps_linear_factors).  Exact for any stiffness: no
// launch, transform or stability limit is added.  nns_spec_ns_linear_spectrum_f32 gives the linear term's rates per shell.
// Measured on the MI355X (profiles/pspec_linear_run.json): linear / steady-forced step 1.016x at 256^2 x 64 and 1.003x at 1024^2 x 8; the
// LINEAR kernels hold 132 ... 151 VGPRs (3 waves per SIMD where most forced twins run 4; profiles/pspec_linear_isa.txt), no scratch.
//
// Reverse mode (nns_spec_ns_step_adjoint_f32; restatement: tests/pspec_adjoint_oracle.py): the vector-Jacobian product of the forced step, last
// step first, in the same layout (cotangents are spectra of real fields paired by the grid sum).  Per step the stage states are recomputed
// from the step's saved start spectrum by the forward's own launches, whose column kernels of stages 1-3 take a trailing PsKeep (STAGES) and
// also store the next stage's input; then ps_col_adj_kernel<nx, S>, S = 4 .. 0, and ps_row_adj_kernel<ny> between them apply N'(s)^T and the
// transposed Lawson update (their notes below).  7 + 9 launches per step; kernels without the PsKeep keep their names and their code.
// Measured on the MI355X (profiles/pspec_adjoint_run.json): adjoint / forward step 2.57x at 256^2 x 64 and 2.72x at 1024^2 x 8; the new kernels
// hold 99 ... 184 VGPRs, no scratch.
//
// Reverse mode of the scalar and the buoyant step (nns_spec_ns_step_scalar_adjoint_f32; restatement: tests/pspec_scalar_adjoint_oracle.py): the
// vector-Jacobian product of the system (w^, theta^), the scalar riding in the flow adjoint's launches as it rides in the step's: still 7 + 9
// per step.  The recomputation is the forward's scalar (b != 0: buoyant) launches, whose column kernels of stages 1-3 take a PsKeepScalar after
// the PsScalar and store the next stage's w^ and theta^; ps_row_adj_kernel<ny, true, PsAdjGrad> runs five inverse transforms and three products
// (the scalar's cotangent joins the vorticity's under the one inverse Laplacian; the buoyancy's adjoint is two multiply-adds in physical space),
// and ps_col_adj_kernel<nx, S, PsAdjScalar> does per tile the vorticity's work, then the scalar's with E_theta and the mask that keeps (0, 0):
// the recurrences have one text for both spectra and both steps (pspec_col_adj_pass.inc).  G has 10 fields there and Ph 3; one host driver
// (spec_ns_step_adjoint) and one table of workspace layouts (PsLayout) serve both entry points.  These kernels hold 108 ... 191 VGPRs, no
// scratch (profiles/pspec_scalar_adjoint_isa.txt; the flow's column kernels after the merge: profiles/pspec_adjoint_unify_isa.txt).
// Measured on the MI355X (profiles/pspec_scalar_adjoint_run.json): adjoint / forward scalar step 2.59x (passive) and 2.48x (buoyant) at
// 256^2 x 64, 2.60x and 2.56x at 1024^2 x 8; adjoint / flow adjoint 1.71x ... 1.73x and 1.79x ... 1.80x, where the byte model (219 against 132
// compacted fields moved per step) says 1.66x.
//
// Reverse mode of the linear step, with or without scalar, buoyancy and noise (nns_spec_ns_step_linear_adjoint_f32; restatement:
// tests/pspec_linear_adjoint_oracle.py): the complex Lawson factor has E(-k) = conj(E(k)), so under the grid sum's pairing its transpose is
// multiplication by conj(E_k), and the recurrences above hold with conj(E) - 1, conj(E^2) - 1 where they have the real em1, em2.  The same driver
// with a table: the recomputation's column kernels of stages 1-3 take the PsLinear before the PsKeep / PsKeepScalar (LINEAR and STAGES
// together), and ps_col_adj_kernel of stages 3-1 takes a PsAdjLinear / PsAdjScalarLinear, whose pass does the forward's 8-byte load and
// ps_linear_factors and negates the imaginary parts; stages 4 and 0, both row kernels and the scalar's real E_theta are untouched, still 7 + 9
// launches per step.  The kick of a stochastic step is additive and independent of the state: its Jacobian is the identity, the saved start
// spectra carry it, and the adjoint of a stochastic step is that of the deterministic step it contains -- no kernel, the generator never runs.
// The new kernels' registers: profiles/pspec_linear_adjoint_isa.txt (no scratch); times: profiles/pspec_linear_adjoint_run.json.
//
// Reverse mode in the linear operator itself (nns_spec_ns_step_operator_adjoint_f32; restatement: tests/pspec_operator_grad_oracle.py): the
// step reads its operator from the table l = lambda dt / 2, so the table is the object to differentiate -- nu, drag, nu_h, mu, beta and any
// learned diagonal operator follow by the chain rule on the host.  The stages' derivatives in l need no N and no division by E, and the
// cotangents they pair with are the ones adjoint stages 3-1 already hold (ps_col_adj_kernel's note): a PsAdjOperator / PsAdjScalarOperator in
// place of the PsAdjLinear / PsAdjScalarLinear makes those three launches also sum c conj(D) per mode and grid, lane-owned like gbar.  The same
// driver, workspaces and 16 launches per step; without lbar the call is the linear adjoint's, launch for launch.  Every other kernel keeps
// its instructions.  Registers and times: profiles/pspec_operator_grad_isa.txt (no scratch), profiles/pspec_operator_grad_run.json.
//
// Forward mode (nns_spec_ns_step_tangent_f32; restatement: tests/pspec_tangent_oracle.py): the Jacobian of the step applied to a perturbation dw^
// that is carried along with the flow.  The Lawson recurrences are linear in (w^, N^), so the tangent step is the same four stages on dw^ with
// the same factors and dN_i = -M [u dw_x + v dw_y + du w_x + dv w_y]^ + dg^ about stage i's own state: a second field that rides in the step's
// launches exactly as the scalar does, with the vorticity's factors and mask where the scalar has E_theta and M_theta.  ps_row_tan_kernel<ny>
// runs four inverse transforms (G fields 0-3 of the base, 4-7 of the perturbation), the base's product with ps_row_kernel's arithmetic and the
// linearised one, and two forward transforms to Ph fields 0 and 1; a PsTangent first in ps_col_kernel's pack (TANGENT) includes
// pspec_col_pass.inc once more per tile (TG) for dw^ / dA -- stage 0, the plain and the forced stages 1-4, the LINEAR stages 1-3, the STOCH
// stages 1 and 4, where the base alone counts the clock and takes the kick.  Still 8 launches per step plus one per call, one driver
// (spec_ns_step) and one more row of PsLayout (12 compacted fields); the base is bitwise the step without the perturbation, and kernels without
// the PsTangent keep their names and their code.  Registers and times: profiles/pspec_tangent_isa.txt (no scratch), profiles/pspec_tangent_run.json.
//
// K tangents on one base (nns_spec_ns_step_tangents_f32; restatement: tests/pspec_lyapunov_oracle.py): dwhat [K][B][my1][nx], member k exactly a
// dwhat of the call above.  u, v, w_x, w_y of a stage are the same for every member, so ps_row_tans_kernel<ny> transforms them once per row
// and keeps both lines while a run-time loop passes the K perturbations through (2 + 2K inverse and 1 + K forward transforms where K calls
// run 4K and 2K; G fields 4+4k .. 7+4k, Ph field 1+k), and a PsTangents first in ps_col_kernel's pack (TANGENTS) runs the TG text K times per
// tile after the vorticity's, on dW + k kstride / dA + k kstride (1 + K passes through a tile against 2K).  Member k's arithmetic is the
// single tangent's, expression for expression.  No dg^ per member.  One more row of PsLayout that depends on K (6 + 6K compacted fields), the
// same driver and launch count; the PsTangent kernels and every kernel without either struct keep their names and their code
// (profiles/pspec_tangents_isa.txt, no scratch; times: profiles/pspec_tangents_run.json).  ps_tangent_gram_kernel is the energy Gram matrix
// of the K members per grid (float64, ps_diag_kernel's fixed order of summation) and ps_tangent_combine_kernel the in-place triangular
// recombination d_k <- sum_{l <= k} C[l][k] d_l: the two halves of a Cholesky QR, whose K x K algebra is the caller's.
//
// Forward mode of the scalar and the buoyant step (nns_spec_ns_step_scalar_tangent_f32; restatement: tests/pspec_scalar_tangent_oracle.py): one
// system (w^, theta^), one tangent (dw^, dtheta^), the same four stages on the pair with dw^ under the vorticity's factors and mask and
// dtheta^ under the scalar's real E_theta and the mask that keeps (0, 0), and about every stage's own state
//     dN_w = -M [u dw_x + v dw_y + du w_x + dv w_y]^ + dg^ + M (i kx by - i ky bx) dtheta^
//     dN_theta = -M_theta [u dtheta_x + v dtheta_y + du (theta_x + Gx) + dv (theta_y + Gy)]^
// The pair rides in the scalar step's launches: ps_row_tan_scalar_kernel<ny, BUOYANT> (its note: seven inverse and four forward transforms,
// three lines live; G fields 0-5 the base's, 6-11 the perturbation's; Ph fields 0, 1 the base's products in ps_row_kernel's arithmetic, 2, 3 the
// linearised ones), and a PsScalar, a PsTangent and a PsTangentScalar together in ps_col_kernel's pack (TANSC) run pspec_col_pass.inc four
// times per tile: w^, theta^, dw^ (TG: Ph field 2, G fields 6-9) and dtheta^ (TH with TG: Ph field 3, G fields 10 and 11, no g^, no dg^, no kick,
// zero means; dN_theta's (0, 0) mode, which vanishes identically, is set to zero, so the mean of dtheta is carried bit for bit) -- stage 0,
// the forced stages 1-4, the LINEAR stages 1-3, the STOCH stages 1 and 4.  These kernels are instantiated in pspec_scalar_tangent.hip (this
// text under PSPEC_SCALAR_TANGENT_TU; ps_scalar_tangent_col / ps_scalar_tangent_row are the way in).  Still 8 launches per step plus one per call, one driver
// (spec_ns_step), one more row of PsLayout (4 accumulators, 12 G, 4 Ph: 20 compacted fields); the base is bitwise the step without the
// perturbation, with b = 0 dw^ is bitwise the flow tangent's, and every other kernel keeps its name and its code.  Registers and times:
// profiles/pspec_scalar_tangent_isa.txt (no scratch), profiles/pspec_scalar_tangent_run.json.
//
// K tangent pairs on one base with a scalar (nns_spec_ns_step_scalar_tangents_f32; restatement: tests/pspec_scalar_lyapunov_oracle.py): dwhat,
// dthat [K][B][my1][nx], member k exactly a pair of the call above with dg^ = NULL.  ps_row_tans_scalar_kernel<ny, BUOYANT> transforms the base's
// three lines once per row and keeps them while a run-time loop passes the K pairs through (3 + 3K inverse and 2 + 2K forward transforms
// where K calls run 7K and 4K; G fields 6+6k .. 11+6k, Ph fields 2+2k, 3+2k), and a PsScalar, a PsTangents and a PsTangentsScalar in
// ps_col_kernel's pack (TANSCS) run the vorticity's pass, the scalar's, then the TANSC form's two tangent passes K times (2 + 2K passes
// through a tile against 4K).  One more row of PsLayout that depends on K (10 + 10K compacted fields), the same driver and launch count.
// These kernels are instantiated in pspec_scalar_tangents.hip (this text under PSPEC_SCALAR_TANGENTS_TU), which also holds
// ps_tangent_variance_gram_kernel, the scalar half of the pairs' inner product; every other kernel keeps its name and its code
// (profiles/pspec_scalar_tangents_isa.txt, no scratch; times: profiles/pspec_scalar_tangents_run.json).
//
// Second-order adjoint (nns_spec_ns_step_second_adjoint_f32; restatement: tests/pspec_second_adjoint_oracle.py): the derivative of the
// reverse mode above in a direction (dw^, dg^, dlam) -- the Hessian-vector product of a loss of the rollout.  N is bilinear, so N'(s)^T kappa is
// linear in s and in kappa, and the derivative of an adjoint stage is
//     dr = N'(s_i)^T dkappa + N'_0(d_i)^T kappa,
// d_i the tangent stage state (that of nns_spec_ns_step_tangent_f32) and N'_0 the same operator with u, v, w_x, w_y of d_i and no mean flow;
// the Lawson recurrences of ps_col_adj_kernel's note are linear, so (dlam, dkappa, dwbar, dgbar) obey them with dr where they have r.  A second
// quadruple that rides in the adjoint's launches: the recomputation is the TANGENT step's (its column kernels of stages 1-3 take a trailing
// PsKeepTangent and store the next stage's w^ and dw^), ps_row_adj2_kernel<ny> runs six inverse and four forward transforms (its note), and a
// PsAdjSecond (PsAdjSecondLinear: the LINEAR twin) makes ps_col_adj_kernel include pspec_col_adj_pass.inc once more per tile (TD) on dlam / dwbar /
// dgbar, Ph fields 2 and 3 and G fields 10 and 11, then prepare the tangent stage's four spectra as G fields 6-9 with zero means.  The first
// quadruple's arithmetic is the adjoint's, so lam and gbar come out bitwise as from nns_spec_ns_step_adjoint_f32 / _linear_adjoint_f32.  Still
// 7 + 9 launches per step, one more row of PsLayout (2 accumulators, 12 G, 4 Ph, 6 kept stages: 24 compacted fields).  The new kernels are
// instantiated in pspec_second_adjoint.hip (this text under PSPEC_SECOND_ADJOINT_TU); every other kernel keeps its name and its code
// (profiles/pspec_second_adjoint_isa.txt, no scratch).
//
// Init / output (not the hot path) use the standalone rfft2 / irfft2 (spectral_ops.hip) plus the pointwise kernels below.
//
// What the row and column kernels share has one copy each: the LDS layout, PsArgs and the row pass's Hermitian fill and kept-mode store in
// pspec_device.h; the line and tile geometry, the staged forward transform and the field emit as text included at each site
// (pspec_row_line.inc, pspec_col_tile.inc, pspec_stage.inc, pspec_field.inc), the way pspec_col_pass.inc and pspec_col_adj_pass.inc serve the vorticity and the scalar:
// a function, a lambda or a type in their place compiles the column kernels to other registers, and their code is pinned
// (tools/isa_listing.py).  The mode predicate (mx, keep, kx, k2) stays spelt out where it is used, for the same reason.
#include "pspec_device.h"
#include <type_traits>
#include <cmath>

// The kernels of the scalar system's tangent are instantiated in a translation unit of their own (pspec_scalar_tangent.hip: this text with
// PSPEC_SCALAR_TANGENT_TU defined, which keeps the host entry points out and these two functions in), so that the two halves compile side by
// side.  The structs of the anonymous namespace have one text, so they cross as untyped pointers: a (PsArgs), fc (PsForce or NULL), sc
// (PsScalar), st (PsStoch or NULL), li (PsLinear or NULL), tg (PsTangent), tt (PsTangentScalar); gr: a PsBuoyGrad (buoyant) or a PsGrad.
int ps_scalar_tangent_col(int nx, int S, const void* Ph, void* G, void* W, void* A, const float* mean, const void* a, int emit, const void* fc,
                          const void* sc, void* stream, const void* st, const void* li, const void* tg, const void* tt);
int ps_scalar_tangent_row(int ny, const void* G, void* Ph, const void* a, void* stream, const void* gr, int buoyant);
// The kernels of K tangents on the scalar system likewise (pspec_scalar_tangents.hip, PSPEC_SCALAR_TANGENTS_TU); ts: PsTangents, tu: PsTangentsScalar.
int ps_scalar_tangents_col(int nx, int S, const void* Ph, void* G, void* W, void* A, const float* mean, const void* a, int emit, const void* fc,
                           const void* sc, void* stream, const void* st, const void* li, const void* ts, const void* tu);
int ps_scalar_tangents_row(int ny, const void* G, void* Ph, const void* a, void* stream, const void* gr, int buoyant, int K);
// The kernels of the second-order adjoint likewise (pspec_second_adjoint.hip, PSPEC_SECOND_ADJOINT_TU); tg: PsTangent, ke: PsKeepTangent, ad: a
// PsAdjSecond, lin: the table of a linear step or NULL (stages 3-1 then take the PsAdjSecondLinear built from ad and lin).
int ps_second_adjoint_col_keep(int nx, int S, const void* Ph, void* G, void* W, void* A, const float* mean, const void* a, const void* fc,
                               const void* li, void* stream, const void* tg, const void* ke);
int ps_second_adjoint_row(int ny, const void* G, void* Ph, const void* a, void* stream);
int ps_second_adjoint_col(int nx, int S, const void* Ph, void* G, const float* mean, const void* a, const void* ad, const void* lin, void* stream);
#if defined(PSPEC_SCALAR_TANGENT_TU) || defined(PSPEC_SCALAR_TANGENTS_TU) || defined(PSPEC_SECOND_ADJOINT_TU)
#define PSPEC_KERNEL_TU      // a translation unit of kernels and their launches alone: no host entry point
#endif

namespace {

constexpr long kGridCap = 2048;

struct PsForce {          // the extra argument of the FORCED column kernels
    const float2* g;      // g^ [gbatch][my1][nx] in the state's layout, or NULL (drag only)
    int shared;           // 1: one g^ for every grid (gbatch = 1); 0: one per grid
    float hdrag;          // alpha dt / 2
};
struct PsNoForce {};

struct PsScalar {         // the extra argument of the SCALAR column kernels
    float2* T;            // theta^ [B][my1][nx], the layout of W
    float2* At;           // its Lawson accumulator
    float hkdt;           // -kappa dt / 2
};
struct PsGrad { float gx, gy; };      // the extra argument of the SCALAR row kernel: the uniform mean gradient
struct PsBuoyGrad {                   // that of the BUOYANT row kernel: the gradient and the buoyancy as the coefficients of G fields 4 and 5
    float gx, gy;
    float c4, c5;                     // -ny by, ny bx
};
struct PsStoch {          // the last argument of the STOCH column kernels (stages 1 and 4 of a stochastic step)
    const float* amp;     // a [my1][nx], the layout of one grid of W, shared by the batch
    unsigned k0, k1;      // the seed's low and high word: the Philox key
    long long* clock;     // [1]: stochastic steps taken; stage 1 advances it, stage 4 reads n = clock - 1
    const int* ids;       // [B]: the grid ids, the fourth counter word
    float sqdt;           // sqrt(dt)
};
struct PsLinear {         // the argument of the LINEAR column kernels (stages 1-3 of a linear step), after PsScalar and before PsStoch
    const float2* lin;    // (Re, Im)(lambda dt / 2) [my1][nx], the layout of one grid of W, shared by the batch
};
struct PsTangent {        // the first extra argument of the TANGENT column kernels (nns_spec_ns_step_tangent_f32); after a PsScalar only with a PsTangentScalar, never with a PsKeep
    float2* dW;           // dw^ [B][my1][nx], the layout of W: the tangent spectrum, advanced with the vorticity's own factors and mask
    float2* dA;           // its Lawson accumulator
    const float2* dg;     // dg^ [dgbatch][my1][nx], the perturbation of the source, or NULL
    int dshared;          // 1: one dg^ for every grid; 0: one per grid
};
struct PsTangentScalar {  // follows a PsScalar and a PsTangent in the pack (nns_spec_ns_step_scalar_tangent_f32): the scalar's perturbation; never with a PsKeep or a PsTangents
    float2* dT;           // dtheta^ [B][my1][nx], the layout of W: advanced with the scalar's E_theta and the mask that keeps (0, 0)
    float2* dAt;          // its Lawson accumulator
};
struct PsTangents {       // the first extra argument of the TANGENTS column kernels (nns_spec_ns_step_tangents_f32): K tangents on one base; after a PsScalar only with a PsTangentsScalar, never with a PsKeep
    float2* dW;           // dw^ [K][B][my1][nx]: member k at dW + k kstride, each in the layout of W
    float2* dA;           // their Lawson accumulators, member k at dA + k kstride
    long kstride;         // complex elements between two members (= B my1 nx)
    int K;                // members, 1 .. 32
};
struct PsTangentsScalar { // follows a PsScalar and a PsTangents in the pack (nns_spec_ns_step_scalar_tangents_f32): the K scalar perturbations; never with a PsKeep or a PsTangent
    float2* dT;           // dtheta^ [K][B][my1][nx]: member k at dT + k kstride (the PsTangents' stride), each advanced as a PsTangentScalar's dT
    float2* dAt;          // their Lawson accumulators, member k at dAt + k kstride
};
struct PsKeep {           // the last argument of the STAGES column kernels (stages 1-3 of the adjoint's recomputation; no scalar or noise)
    float2* stage;        // [B][my1][nx], the layout of W: receives the next stage's input spectrum (s1, s2 or s3)
};
struct PsKeepScalar {     // PsKeep of the SCALAR kernels (after PsScalar): the adjoint of the scalar and the buoyant step recomputes both spectra
    float2* stage;        // [B][my1][nx]: the next stage's w^
    float2* tstage;       // [B][my1][nx]: the next stage's theta^
};
struct PsKeepTangent {    // PsKeep of the TANGENT kernels (last in the pack, after the PsLinear of a linear step): the second-order adjoint recomputes both spectra
    float2* stage;        // [B][my1][nx]: the next stage's w^
    float2* dstage;       // [B][my1][nx]: the next stage's dw^
};
struct PsAdj {            // the argument of the adjoint column kernels
    float2* lam;          // [B][my1][nx]: the cotangent of the step's result; stage 0 writes the cotangent of its input over it
    float2* wbar;         // [B][my1][nx]: the cotangent of the step's input while it is summed (stages 3..0)
    float2* gbar;         // [B][my1][nx] or NULL: the cotangent of g^, summed over stages and steps
    const float2* state;  // [B][my1][nx]: the stage state the NEXT adjoint stage linearises about (S = 4: s3, 3: s2, 2: s1, 1: s0), unused by S = 0
    float hdrag;          // alpha dt / 2
    int ginit;            // S = 4: 1 starts gbar (the first step a call takes), 0 adds to it
};
struct PsAdjScalar : PsAdj {      // with a scalar: PsAdj and its twin for theta^ (no source, so no gbar of its own)
    float2* mu;          // [B][my1][nx]: the cotangent of the step's theta^; stage 0 writes the cotangent of its input over it
    float2* tbar;         // [B][my1][nx]: the cotangent of the step's input theta^ while it is summed (stages 3..0)
    const float2* tstate; // [B][my1][nx]: theta^ of the stage state that state belongs to
    float hkdt;           // -kappa dt / 2
};
struct PsAdjLinear : PsAdj {      // the LINEAR adjoint column kernels (stages 3-1 of a linear step's adjoint): PsAdj and the forward's table
    const float2* lin;    // (Re, Im)(lambda dt / 2) [my1][nx], as PsLinear's: the factors are conj(E), conj(E^2); a.hnudt and hdrag are then unused
};
struct PsAdjScalarLinear : PsAdjScalar {      // the same with a scalar, whose own factor stays the real E_theta
    const float2* lin;
};
struct PsAdjOperator : PsAdjLinear {          // the LINEAR kernels that also sum the table's cotangent (nns_spec_ns_step_operator_adjoint_f32)
    float2* lbar;         // [B][my1][nx]: the cotangent of lin per grid before weight and symmetrisation, summed over the steps: stage 1 adds the
                          // step's sum to it, or starts it where ginit is set
    float2* lstep;        // [B][my1][nx]: the step's own sum while it is made (stage 3 writes it, stage 2 adds, stage 1 reads)
    const float2* own;    // [B][my1][nx]: the state THIS stage's r belongs to (S = 3: s3, 2: s2, 1: s1)
    const float2* w0;     // [B][my1][nx]: the step's start spectrum (read by S = 3 and 2)
};
struct PsAdjScalarOperator : PsAdjScalarLinear {      // the same with a scalar, whose E_theta is a constant
    float2* lbar;
    float2* lstep;
    const float2* own;
    const float2* w0;
};
struct PsAdjSecond : PsAdj {      // the second-order adjoint (nns_spec_ns_step_second_adjoint_f32): PsAdj and its twin for the derivative in the direction
    float2* dlam;         // [B][my1][nx]: the derivative of lam; stage 0 writes that of the cotangent of the step's input over it
    float2* dwbar;        // [B][my1][nx]: the derivative of wbar while it is summed (stages 3..0)
    float2* dgbar;        // [B][my1][nx] or NULL: the derivative of gbar, summed over stages and steps (ginit starts it, as it starts gbar)
    const float2* dstate; // [B][my1][nx]: the tangent stage state that belongs to state (S = 4: d3, 3: d2, 2: d1, 1: d0), unused by S = 0
};
struct PsAdjSecondLinear : PsAdjSecond {      // its LINEAR form (stages 3-1 of a linear step): both quadruples take conj(E), conj(E^2) from the table
    const float2* lin;
};
struct PsAdjGrad {        // the argument of the scalar adjoint row kernel: the uniform mean gradient and the buoyancy
    float gx, gy, bx, by;
};
template <typename U, typename T, typename... R> __device__ __forceinline__ U pick(T t, R... r) {           // the pack's element of type U
    if constexpr (std::is_same_v<U, T>) return t;
    else return pick<U>(r...);
}

__device__ __forceinline__ cf scal(cf em, cf z) {                                                            // (1 + em) z, em complex
    return {fmaf(-em.y, z.y, fmaf(em.x, z.x, z.x)), fmaf(em.y, z.x, fmaf(em.x, z.y, z.y))};
}

// E - 1 and E^2 - 1 of E = exp(x + i phi), l = (x, phi) = lambda dt / 2, in the z + (E - 1) z form of the real factors: with the half angle
// (sh, ch) = sincos(phi / 2), t = 2 sh^2 = 1 - cos phi and s = 2 sh ch = sin phi,
//     Re(E - 1) = expm1(x) cos phi - 2 sin^2(phi / 2) = expm1(x) (1 - t) - t,      Im(E - 1) = exp(x) sin phi = expm1(x) s + s
// (no cancellation for small phi; phi = 0 gives the real factor exactly), and E^2 - 1 = (E - 1)(E + 1) from e = E - 1:
//     Re = e.x (e.x + 2) - e.y^2 = |E|^2 cos^2 phi - 1 - e.y^2 (two terms <= 0 for x <= 0: they cannot cancel),      Im = 2 e.y (e.x + 1)
// sincospif reduces its argument exactly, so a large phi costs nothing and loses only the rounding of phi / pi.
__device__ __forceinline__ void ps_linear_factors(float2 l, cf& e1, cf& e2) {
    float sh, ch;
    sincospif(l.y * 0.15915494309189535f, &sh, &ch);                  // phi / 2 in units of pi
    const float s = 2.f * sh * ch, t = 2.f * sh * sh;
    const float x1 = expm1f(l.x);
    e1 = {fmaf(x1, 1.f - t, -t), fmaf(x1, s, s)};
    e2 = {fmaf(e1.x, e1.x + 2.f, -e1.y * e1.y), 2.f * e1.y * (e1.x + 1.f)};
}

// Philox4x32-10 (Salmon et al., SC'11), outputs 0 and 1 of counter (c0, c1, c2, c3) under key (k0, k1), mapped to one complex standard normal
// with E |xi|^2 = 1: u1 = ((x0 >> 8) + 1) 2^-24 in (0, 1], u2 = (x1 >> 8) 2^-24 in [0, 1), xi = sqrt(-ln u1) (cos 2 pi u2, sin 2 pi u2).
// 2 u2 is exact in float32 and sincospif reduces its argument exactly.
__device__ __forceinline__ cf ps_normal(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    const float u1 = (float)((c0 >> 8) + 1u) * 0x1p-24f, u2 = (float)(c1 >> 8) * 0x1p-24f;
    const float rad = sqrtf(-logf(u1));
    float sn, cs;
    sincospif(2.f * u2, &sn, &cs);
    return {rad * cs, rad * sn};
}

// ---------------------------------------------------------------------------------------------------- row pass (axis y)
// SCALAR: a third inverse transform (theta_x + i theta_y, G fields 4 and 5) after the vorticity's product has left, so two complex lines
// are live at a time, as without it; the second product goes to Ph's second field.
// BUOYANT (SCALAR only): c4 G4 + c5 G5 of the row's kept y-modes joins the vorticity's transformed product on its way to Ph.
template <int N, bool SCALAR = false, bool BUOYANT = false, typename... Grad>
__global__ __launch_bounds__(kT) void ps_row_kernel(const float2* __restrict__ G, float2* __restrict__ Ph, PsArgs a, Grad... grad) {
    static_assert(sizeof...(Grad) == (SCALAR ? 1 : 0), "the gradient is the SCALAR kernel's argument");
    static_assert(SCALAR || !BUOYANT, "buoyancy needs the scalar");
    using L = PsLds<N>;
    constexpr int TPF = L::TPF;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const cf* tab = ps_tables<N>(smem);
    unsigned char* lines = smem + L::TAB_BYTES;
    const int my1 = a.my1;
    const long niter = (a.nlines + L::LINES - 1) / L::LINES;
    for (long it = blockIdx.x; it < niter; it += gridDim.x) {
#include "pspec_row_line.inc"
        cf zu[16], zw[16];
        ps_row_load2<N>(g0, g0 + a.fstride, tid, my1, zu);                       // u + i v
        fft_line<float, N, true>(zu, tab, tab + N / 2, xb, tid);
        __builtin_amdgcn_sched_barrier(0);
        ps_row_load2<N>(g0 + 2 * a.fstride, g0 + 3 * a.fstride, tid, my1, zw);   // w_x + i w_y
        fft_line<float, N, true>(zw, tab, tab + N / 2, xb, tid);
        if constexpr (!SCALAR) {
#pragma unroll
            for (int m = 0; m < 16; ++m) zu[m] = {zu[m].x * zw[m].x + zu[m].y * zw[m].y, 0.f};    // u w_x + v w_y
            __builtin_amdgcn_sched_barrier(0);
            fft_line<float, N, false>(zu, tab, tab + N / 2, xb, tid);
            ps_row_store<N>(zu, Ph + (size_t)row * my1, tid, my1, valid);
        } else {
            const auto gr = pick<Grad...>(grad...);
#pragma unroll
            for (int m = 0; m < 16; ++m) zw[m] = {zu[m].x * zw[m].x + zu[m].y * zw[m].y, 0.f};    // u w_x + v w_y: u, v stay
            __builtin_amdgcn_sched_barrier(0);
            fft_line<float, N, false>(zw, tab, tab + N / 2, xb, tid);
            if constexpr (BUOYANT) {                             // -ny (by theta_x - bx theta_y)^ on the kept modes: the loads of load2 below
                const float2* t4 = g0 + 4 * a.fstride;
                const float2* t5 = g0 + 5 * a.fstride;
#pragma unroll
                for (int m = 0; m < 8; ++m) {
                    const int e = tid + TPF * m;
                    if (e < my1) {
                        const float2 p = t4[e], q = t5[e];
                        zw[m] = {fmaf(gr.c4, p.x, fmaf(gr.c5, q.x, zw[m].x)), fmaf(gr.c4, p.y, fmaf(gr.c5, q.y, zw[m].y))};
                    }
                }
            }
            ps_row_store<N>(zw, Ph + (size_t)row * my1, tid, my1, valid);
            __builtin_amdgcn_sched_barrier(0);
            ps_row_load2<N>(g0 + 4 * a.fstride, g0 + 5 * a.fstride, tid, my1, zw);   // theta_x + i theta_y
            fft_line<float, N, true>(zw, tab, tab + N / 2, xb, tid);
#pragma unroll
            for (int m = 0; m < 16; ++m) zw[m] = {zu[m].x * (zw[m].x + gr.gx) + zu[m].y * (zw[m].y + gr.gy), 0.f};   // u (theta_x + Gx) + v (theta_y + Gy)
            __builtin_amdgcn_sched_barrier(0);
            fft_line<float, N, false>(zw, tab, tab + N / 2, xb, tid);
            ps_row_store<N>(zw, Ph + a.fstride + (size_t)row * my1, tid, my1, valid);
        }
    }
}

// The row pass of the tangent-linear step (nns_spec_ns_step_tangent_f32; restatement: tests/pspec_tangent_oracle.py).  The perturbation dw^
// rides in the step's launches as the scalar does: G fields 4-7 hold its velocity and gradient (du, dv, dw_x, dw_y: no mean flow), and beside
// the base's product u w_x + v w_y (Ph field 0: the arithmetic of ps_row_kernel, so the base stays bitwise the step) the row forms the
// linearised one, u dw_x + v dw_y + du w_x + dv w_y (Ph field 1).  Four inverse and two forward transforms along y.  u + i v and
// w_x + i w_y stay while one perturbation line at a time passes: du w_x + dv w_y is formed first, as 16 real values that take the place of
// w_x + i w_y, and the same line then carries grad dw.  Three complex lines are live, as in ps_row_adj_kernel<N, true>.
template <int N>
__global__ __launch_bounds__(kT) void ps_row_tan_kernel(const float2* __restrict__ G, float2* __restrict__ Ph, PsArgs a) {
    using L = PsLds<N>;
    constexpr int TPF = L::TPF;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const cf* tab = ps_tables<N>(smem);
    unsigned char* lines = smem + L::TAB_BYTES;
    const int my1 = a.my1;
    const long niter = (a.nlines + L::LINES - 1) / L::LINES;
    for (long it = blockIdx.x; it < niter; it += gridDim.x) {
#include "pspec_row_line.inc"
        cf zu[16], zw[16], zd[16];
        ps_row_load2<N>(g0, g0 + a.fstride, tid, my1, zu);                           // u + i v: stays
        fft_line<float, N, true>(zu, tab, tab + N / 2, xb, tid);
        __builtin_amdgcn_sched_barrier(0);
        ps_row_load2<N>(g0 + 2 * a.fstride, g0 + 3 * a.fstride, tid, my1, zw);       // w_x + i w_y: stays
        fft_line<float, N, true>(zw, tab, tab + N / 2, xb, tid);
#pragma unroll
        for (int m = 0; m < 16; ++m) zd[m] = {zu[m].x * zw[m].x + zu[m].y * zw[m].y, 0.f};        // u w_x + v w_y
        __builtin_amdgcn_sched_barrier(0);
        fft_line<float, N, false>(zd, tab, tab + N / 2, xb, tid);
        ps_row_store<N>(zd, Ph + (size_t)row * my1, tid, my1, valid);
        __builtin_amdgcn_sched_barrier(0);
        ps_row_load2<N>(g0 + 4 * a.fstride, g0 + 5 * a.fstride, tid, my1, zd);       // du + i dv
        fft_line<float, N, true>(zd, tab, tab + N / 2, xb, tid);
#pragma unroll
        for (int m = 0; m < 16; ++m) zw[m].x = zd[m].x * zw[m].x + zd[m].y * zw[m].y;             // du w_x + dv w_y: w_x, w_y leave
        __builtin_amdgcn_sched_barrier(0);
        ps_row_load2<N>(g0 + 6 * a.fstride, g0 + 7 * a.fstride, tid, my1, zd);       // dw_x + i dw_y
        fft_line<float, N, true>(zd, tab, tab + N / 2, xb, tid);
#pragma unroll
        for (int m = 0; m < 16; ++m) zd[m] = {fmaf(zu[m].x, zd[m].x, fmaf(zu[m].y, zd[m].y, zw[m].x)), 0.f};   // + u dw_x + v dw_y
        __builtin_amdgcn_sched_barrier(0);
        fft_line<float, N, false>(zd, tab, tab + N / 2, xb, tid);
        ps_row_store<N>(zd, Ph + a.fstride + (size_t)row * my1, tid, my1, valid);
    }
}

// The row pass of the tangent of the scalar system (nns_spec_ns_step_scalar_tangent_f32; restatement: tests/pspec_scalar_tangent_oracle.py):
// ps_row_tan_kernel's twin, as ps_row_kernel<N, true, BUOYANT> is ps_row_kernel<N>'s.  G fields 0-5 are the base's (u, v, w_x, w_y, theta_x,
// theta_y), 6-11 the perturbation's (du, dv, dw_x, dw_y, dtheta_x, dtheta_y: no mean flow); Ph fields 0 and 1 take the base's two products,
// spelt with ps_row_kernel<N, true, BUOYANT>'s arithmetic so that the base stays bitwise the step, 2 and 3 the linearised ones,
//     u dw_x + v dw_y + du w_x + dv w_y     and     u dtheta_x + v dtheta_y + du (theta_x + Gx) + dv (theta_y + Gy).
// BUOYANT adds c4 G10 + c5 G11 on the kept modes to the first on its way to Ph, the way it adds G4, G5 to the base's.
// The order taken: SEVEN inverse transforms (du + i dv twice) and four forward ones, with three complex lines live at any moment, as in
// ps_row_tan_kernel: u + i v stays, the second line holds a gradient of the base (grad w, then grad theta) until du, dv have turned it into 16
// reals, the third is the line in flight.  Six inverse transforms are the minimum, but they want a fourth line while grad theta comes in
// (u + i v, du + i dv, the packed partial products, the incoming line): 32 more registers across a transform in a kernel that runs two waves
// per SIMD either way, for one transform in eleven whose input (G fields 6 and 7 of the row) was read a few hundred instructions before.
template <int N, bool BUOYANT>
__global__ __launch_bounds__(kT) void ps_row_tan_scalar_kernel(const float2* __restrict__ G, float2* __restrict__ Ph, PsArgs a,
                                                               std::conditional_t<BUOYANT, PsBuoyGrad, PsGrad> gr) {
    using L = PsLds<N>;
    constexpr int TPF = L::TPF;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const cf* tab = ps_tables<N>(smem);
    unsigned char* lines = smem + L::TAB_BYTES;
    const int my1 = a.my1;
    const long niter = (a.nlines + L::LINES - 1) / L::LINES;
    for (long it = blockIdx.x; it < niter; it += gridDim.x) {
#include "pspec_row_line.inc"
        cf zu[16], zw[16], zd[16];
        ps_row_load2<N>(g0, g0 + a.fstride, tid, my1, zu);                           // u + i v: stays
        fft_line<float, N, true>(zu, tab, tab + N / 2, xb, tid);
        __builtin_amdgcn_sched_barrier(0);
        ps_row_load2<N>(g0 + 2 * a.fstride, g0 + 3 * a.fstride, tid, my1, zw);       // w_x + i w_y: stays until du, dv have met it
        fft_line<float, N, true>(zw, tab, tab + N / 2, xb, tid);
#pragma unroll
        for (int m = 0; m < 16; ++m) zd[m] = {zu[m].x * zw[m].x + zu[m].y * zw[m].y, 0.f};        // u w_x + v w_y
        __builtin_amdgcn_sched_barrier(0);
        fft_line<float, N, false>(zd, tab, tab + N / 2, xb, tid);
        if constexpr (BUOYANT) {                                 // -ny (by theta_x - bx theta_y)^ on the kept modes, as in ps_row_kernel
            const float2* t4 = g0 + 4 * a.fstride;
            const float2* t5 = g0 + 5 * a.fstride;
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const int e = tid + TPF * m;
                if (e < my1) {
                    const float2 p = t4[e], q = t5[e];
                    zd[m] = {fmaf(gr.c4, p.x, fmaf(gr.c5, q.x, zd[m].x)), fmaf(gr.c4, p.y, fmaf(gr.c5, q.y, zd[m].y))};
                }
            }
        }
        ps_row_store<N>(zd, Ph + (size_t)row * my1, tid, my1, valid);
        __builtin_amdgcn_sched_barrier(0);
        ps_row_load2<N>(g0 + 6 * a.fstride, g0 + 7 * a.fstride, tid, my1, zd);       // du + i dv
        fft_line<float, N, true>(zd, tab, tab + N / 2, xb, tid);
#pragma unroll
        for (int m = 0; m < 16; ++m) zw[m].x = zd[m].x * zw[m].x + zd[m].y * zw[m].y;             // du w_x + dv w_y: w_x, w_y leave
        __builtin_amdgcn_sched_barrier(0);
        ps_row_load2<N>(g0 + 8 * a.fstride, g0 + 9 * a.fstride, tid, my1, zd);       // dw_x + i dw_y
        fft_line<float, N, true>(zd, tab, tab + N / 2, xb, tid);
#pragma unroll
        for (int m = 0; m < 16; ++m) zd[m] = {fmaf(zu[m].x, zd[m].x, fmaf(zu[m].y, zd[m].y, zw[m].x)), 0.f};   // + u dw_x + v dw_y
        __builtin_amdgcn_sched_barrier(0);
        fft_line<float, N, false>(zd, tab, tab + N / 2, xb, tid);
        if constexpr (BUOYANT) {                                 // the buoyancy of the scalar's perturbation: G fields 10 and 11 of the row
            const float2* t4 = g0 + 10 * a.fstride;
            const float2* t5 = g0 + 11 * a.fstride;
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const int e = tid + TPF * m;
                if (e < my1) {
                    const float2 p = t4[e], q = t5[e];
                    zd[m] = {fmaf(gr.c4, p.x, fmaf(gr.c5, q.x, zd[m].x)), fmaf(gr.c4, p.y, fmaf(gr.c5, q.y, zd[m].y))};
                }
            }
        }
        ps_row_store<N>(zd, Ph + 2 * a.fstride + (size_t)row * my1, tid, my1, valid);
        __builtin_amdgcn_sched_barrier(0);
        ps_row_load2<N>(g0 + 4 * a.fstride, g0 + 5 * a.fstride, tid, my1, zw);       // theta_x + i theta_y: stays until du, dv have met it
        fft_line<float, N, true>(zw, tab, tab + N / 2, xb, tid);
#pragma unroll
        for (int m = 0; m < 16; ++m) zd[m] = {zu[m].x * (zw[m].x + gr.gx) + zu[m].y * (zw[m].y + gr.gy), 0.f};   // u (theta_x + Gx) + v (theta_y + Gy)
        __builtin_amdgcn_sched_barrier(0);
        fft_line<float, N, false>(zd, tab, tab + N / 2, xb, tid);
        ps_row_store<N>(zd, Ph + a.fstride + (size_t)row * my1, tid, my1, valid);
        __builtin_amdgcn_sched_barrier(0);
        ps_row_load2<N>(g0 + 6 * a.fstride, g0 + 7 * a.fstride, tid, my1, zd);       // du + i dv once more
        fft_line<float, N, true>(zd, tab, tab + N / 2, xb, tid);
#pragma unroll
        for (int m = 0; m < 16; ++m) zw[m].x = zd[m].x * (zw[m].x + gr.gx) + zd[m].y * (zw[m].y + gr.gy);   // du (theta_x + Gx) + dv (theta_y + Gy)
        __builtin_amdgcn_sched_barrier(0);
        ps_row_load2<N>(g0 + 10 * a.fstride, g0 + 11 * a.fstride, tid, my1, zd);     // dtheta_x + i dtheta_y
        fft_line<float, N, true>(zd, tab, tab + N / 2, xb, tid);
#pragma unroll
        for (int m = 0; m < 16; ++m) zd[m] = {fmaf(zu[m].x, zd[m].x, fmaf(zu[m].y, zd[m].y, zw[m].x)), 0.f};   // + u dtheta_x + v dtheta_y
        __builtin_amdgcn_sched_barrier(0);
        fft_line<float, N, false>(zd, tab, tab + N / 2, xb, tid);
        ps_row_store<N>(zd, Ph + 3 * a.fstride + (size_t)row * my1, tid, my1, valid);
    }
}

// The row pass of K tangents on one base (nns_spec_ns_step_tangents_f32).  u + i v and w_x + i w_y are transformed once and stay for the whole
// row; the base's product leaves first (Ph field 0, ps_row_kernel's arithmetic).  Then a run-time loop over the members: du + i dv (G fields
// 4+4k, 5+4k), the 16 reals du w_x + dv w_y (zp: w_x, w_y must survive for the next member, so they are not overwritten as in
// ps_row_tan_kernel), dw_x + i dw_y (6+4k, 7+4k) into the same line, the linearised product spelt as there -- member k's bits are the single
// tangent's -- and its forward transform to Ph field 1+k.  Three and a half complex lines are live; nothing is indexed by k but pointers.
// 162 ... 176 VGPRs, 2 waves per SIMD (3 at N = 512), no scratch.
template <int N>
__global__ __launch_bounds__(kT) void ps_row_tans_kernel(const float2* __restrict__ G, float2* __restrict__ Ph, PsArgs a, int K) {
    using L = PsLds<N>;
    constexpr int TPF = L::TPF;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const cf* tab = ps_tables<N>(smem);
    unsigned char* lines = smem + L::TAB_BYTES;
    const int my1 = a.my1;
    const long niter = (a.nlines + L::LINES - 1) / L::LINES;
    for (long it = blockIdx.x; it < niter; it += gridDim.x) {
#include "pspec_row_line.inc"
        cf zu[16], zw[16], zd[16];
        float zp[16];
        ps_row_load2<N>(g0, g0 + a.fstride, tid, my1, zu);                           // u + i v: stays
        fft_line<float, N, true>(zu, tab, tab + N / 2, xb, tid);
        __builtin_amdgcn_sched_barrier(0);
        ps_row_load2<N>(g0 + 2 * a.fstride, g0 + 3 * a.fstride, tid, my1, zw);       // w_x + i w_y: stays
        fft_line<float, N, true>(zw, tab, tab + N / 2, xb, tid);
#pragma unroll
        for (int m = 0; m < 16; ++m) zd[m] = {zu[m].x * zw[m].x + zu[m].y * zw[m].y, 0.f};        // u w_x + v w_y
        __builtin_amdgcn_sched_barrier(0);
        fft_line<float, N, false>(zd, tab, tab + N / 2, xb, tid);
        ps_row_store<N>(zd, Ph + (size_t)row * my1, tid, my1, valid);
        const float2* gk = g0 + 4 * a.fstride;                                       // member k's four fields
        float2* pk = Ph + a.fstride + (size_t)row * my1;                             // and its Ph field
        for (int k = 0; k < K; ++k, gk += 4 * a.fstride, pk += a.fstride) {
            // the lane's index pinned per turn: what the loads, the transforms and the store derive from it (element offsets, predicates,
            // twiddle addresses) is otherwise hoisted out of the loop and held across it -- 301 ... 313 registers and one wave per SIMD
            // where this takes 162 ... 176
            int tk = tid;
            asm volatile("" : "+v"(tk));
            __builtin_amdgcn_sched_barrier(0);
            ps_row_load2<N>(gk, gk + a.fstride, tk, my1, zd);                        // du + i dv
            fft_line<float, N, true>(zd, tab, tab + N / 2, xb, tk);
#pragma unroll
            for (int m = 0; m < 16; ++m) zp[m] = zd[m].x * zw[m].x + zd[m].y * zw[m].y;           // du w_x + dv w_y: w_x, w_y stay
            __builtin_amdgcn_sched_barrier(0);
            ps_row_load2<N>(gk + 2 * a.fstride, gk + 3 * a.fstride, tk, my1, zd);    // dw_x + i dw_y
            fft_line<float, N, true>(zd, tab, tab + N / 2, xb, tk);
#pragma unroll
            for (int m = 0; m < 16; ++m) zd[m] = {fmaf(zu[m].x, zd[m].x, fmaf(zu[m].y, zd[m].y, zp[m])), 0.f};   // + u dw_x + v dw_y
            __builtin_amdgcn_sched_barrier(0);
            fft_line<float, N, false>(zd, tab, tab + N / 2, xb, tk);
            ps_row_store<N>(zd, pk, tk, my1, valid);
        }
    }
}

// The row pass of K tangent pairs on one base with a scalar (nns_spec_ns_step_scalar_tangents_f32): ps_row_tans_kernel's loop around
// ps_row_tan_scalar_kernel's arithmetic.  G fields 0-5 are the base's, member k's (du, dv, dw_x, dw_y, dtheta_x, dtheta_y) are 6+6k .. 11+6k; Ph
// fields 0 and 1 take the base's two products, 2+2k and 3+2k member k's linearised ones.  u + i v, w_x + i w_y and theta_x + i theta_y are
// transformed once per row and stay; the base's products leave first, spelt as in ps_row_tan_scalar_kernel (so as in ps_row_kernel<N, true,
// BUOYANT>: the base stays bitwise the step).  Then the run-time loop: du + i dv transformed ONCE per member and turned into the 16 reals
// du w_x + dv w_y (zp) and the 16 reals du (theta_x + Gx) + dv (theta_y + Gy) (zq); dw_x + i dw_y, its product, forward, BUOYANT's c4 G[10+6k] +
// c5 G[11+6k], Ph 2+2k; dtheta_x + i dtheta_y, its product, forward, Ph 3+2k.  Every product is spelt as in ps_row_tan_scalar_kernel and a
// transform of the same input gives the same bits, so member k's bits are that kernel's.  3 + 3K inverse and 2 + 2K forward transforms per
// row where K single calls run 7K and 4K.  Four complex lines and 32 reals are live; nothing is indexed by k but pointers, and the lane's
// index is pinned per turn as in ps_row_tans_kernel.
template <int N, bool BUOYANT>
__global__ __launch_bounds__(kT) void ps_row_tans_scalar_kernel(const float2* __restrict__ G, float2* __restrict__ Ph, PsArgs a,
                                                                std::conditional_t<BUOYANT, PsBuoyGrad, PsGrad> gr, int K) {
    using L = PsLds<N>;
    constexpr int TPF = L::TPF;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const cf* tab = ps_tables<N>(smem);
    unsigned char* lines = smem + L::TAB_BYTES;
    const int my1 = a.my1;
    const long niter = (a.nlines + L::LINES - 1) / L::LINES;
    for (long it = blockIdx.x; it < niter; it += gridDim.x) {
#include "pspec_row_line.inc"
        cf zu[16], zw[16], zt[16], zd[16];
        float zp[16], zq[16];
        ps_row_load2<N>(g0, g0 + a.fstride, tid, my1, zu);                           // u + i v: stays
        fft_line<float, N, true>(zu, tab, tab + N / 2, xb, tid);
        __builtin_amdgcn_sched_barrier(0);
        ps_row_load2<N>(g0 + 2 * a.fstride, g0 + 3 * a.fstride, tid, my1, zw);       // w_x + i w_y: stays
        fft_line<float, N, true>(zw, tab, tab + N / 2, xb, tid);
#pragma unroll
        for (int m = 0; m < 16; ++m) zd[m] = {zu[m].x * zw[m].x + zu[m].y * zw[m].y, 0.f};        // u w_x + v w_y
        __builtin_amdgcn_sched_barrier(0);
        fft_line<float, N, false>(zd, tab, tab + N / 2, xb, tid);
        if constexpr (BUOYANT) {                                 // -ny (by theta_x - bx theta_y)^ on the kept modes, as in ps_row_kernel
            const float2* t4 = g0 + 4 * a.fstride;
            const float2* t5 = g0 + 5 * a.fstride;
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const int e = tid + TPF * m;
                if (e < my1) {
                    const float2 p = t4[e], q = t5[e];
                    zd[m] = {fmaf(gr.c4, p.x, fmaf(gr.c5, q.x, zd[m].x)), fmaf(gr.c4, p.y, fmaf(gr.c5, q.y, zd[m].y))};
                }
            }
        }
        ps_row_store<N>(zd, Ph + (size_t)row * my1, tid, my1, valid);
        __builtin_amdgcn_sched_barrier(0);
        ps_row_load2<N>(g0 + 4 * a.fstride, g0 + 5 * a.fstride, tid, my1, zt);       // theta_x + i theta_y: stays
        fft_line<float, N, true>(zt, tab, tab + N / 2, xb, tid);
#pragma unroll
        for (int m = 0; m < 16; ++m) zd[m] = {zu[m].x * (zt[m].x + gr.gx) + zu[m].y * (zt[m].y + gr.gy), 0.f};   // u (theta_x + Gx) + v (theta_y + Gy)
        __builtin_amdgcn_sched_barrier(0);
        fft_line<float, N, false>(zd, tab, tab + N / 2, xb, tid);
        ps_row_store<N>(zd, Ph + a.fstride + (size_t)row * my1, tid, my1, valid);
        const float2* gk = g0 + 6 * a.fstride;                                       // member k's six fields
        float2* pk = Ph + 2 * a.fstride + (size_t)row * my1;                         // and its two Ph fields
        for (int k = 0; k < K; ++k, gk += 6 * a.fstride, pk += 2 * a.fstride) {
            int tk = tid;                                                            // ps_row_tans_kernel's pin
            asm volatile("" : "+v"(tk));
            __builtin_amdgcn_sched_barrier(0);
            ps_row_load2<N>(gk, gk + a.fstride, tk, my1, zd);                        // du + i dv, once
            fft_line<float, N, true>(zd, tab, tab + N / 2, xb, tk);
#pragma unroll
            for (int m = 0; m < 16; ++m) zp[m] = zd[m].x * zw[m].x + zd[m].y * zw[m].y;           // du w_x + dv w_y: w_x, w_y stay
#pragma unroll
            for (int m = 0; m < 16; ++m) zq[m] = zd[m].x * (zt[m].x + gr.gx) + zd[m].y * (zt[m].y + gr.gy);   // du (theta_x + Gx) + dv (theta_y + Gy)
            __builtin_amdgcn_sched_barrier(0);
            ps_row_load2<N>(gk + 2 * a.fstride, gk + 3 * a.fstride, tk, my1, zd);    // dw_x + i dw_y
            fft_line<float, N, true>(zd, tab, tab + N / 2, xb, tk);
#pragma unroll
            for (int m = 0; m < 16; ++m) zd[m] = {fmaf(zu[m].x, zd[m].x, fmaf(zu[m].y, zd[m].y, zp[m])), 0.f};   // + u dw_x + v dw_y
            __builtin_amdgcn_sched_barrier(0);
            fft_line<float, N, false>(zd, tab, tab + N / 2, xb, tk);
            if constexpr (BUOYANT) {                             // the buoyancy of member k's scalar perturbation: its G fields 10+6k and 11+6k
                const float2* t4 = gk + 4 * a.fstride;
                const float2* t5 = gk + 5 * a.fstride;
#pragma unroll
                for (int m = 0; m < 8; ++m) {
                    const int e = tk + TPF * m;
                    if (e < my1) {
                        const float2 p = t4[e], q = t5[e];
                        zd[m] = {fmaf(gr.c4, p.x, fmaf(gr.c5, q.x, zd[m].x)), fmaf(gr.c4, p.y, fmaf(gr.c5, q.y, zd[m].y))};
                    }
                }
            }
            ps_row_store<N>(zd, pk, tk, my1, valid);
            __builtin_amdgcn_sched_barrier(0);
            ps_row_load2<N>(gk + 4 * a.fstride, gk + 5 * a.fstride, tk, my1, zd);    // dtheta_x + i dtheta_y
            fft_line<float, N, true>(zd, tab, tab + N / 2, xb, tk);
#pragma unroll
            for (int m = 0; m < 16; ++m) zd[m] = {fmaf(zu[m].x, zd[m].x, fmaf(zu[m].y, zd[m].y, zq[m])), 0.f};   // + u dtheta_x + v dtheta_y
            __builtin_amdgcn_sched_barrier(0);
            fft_line<float, N, false>(zd, tab, tab + N / 2, xb, tk);
            ps_row_store<N>(zd, pk + a.fstride, tk, my1, valid);
        }
    }
}

// ---------------------------------------------------------------------------------------------------- column pass (axis x)
// S = 0: prepare stage 1 from W; S = 1..4: consume the RK stage's N (from Ph) and update W / A, then (S < 4 or emit) prepare the next stage.
// FORCED (S >= 1): N^ += g^ on the kept modes (lane-owned, coalesced, like W / A) and L dt / 2 = hnudt |k|^2 - alpha dt / 2.
// SCALAR: after the vorticity's work on a tile the same sequence runs once more on the scalar: Ph's second field, theta^ / A_theta with
// L dt / 2 = hkdt |k|^2 (no drag, no force) and a mask that keeps the (0, 0) mode, then G fields 4 and 5.  One field's registers at a time.
// STOCH (a PsStoch ends the pack; FORCED, S = 1 or 4): S = 1 advances the step count, S = 4 adds the kick to the vorticity's w^ (not the scalar's).
// LINEAR (a PsLinear in the pack, after PsScalar, before PsStoch; FORCED, S = 1..3): the vorticity's L dt / 2 is the complex table entry
// lin[j][i], not hnudt |k|^2 - alpha dt / 2 (a.hnudt and fc.hdrag are then unused); the scalar's stays hkdt |k|^2.
// STAGES (a PsKeep ends the pack, after the PsLinear of a linear step; S = 1..3): the next stage's input spectrum is also stored, lane-owned and coalesced like W / A, for the
// adjoint (ps_col_adj_kernel) to linearise about; the arithmetic is untouched, so the recomputed stages are the forward's bits.  With a scalar
// the pack ends in a PsKeepScalar after the PsScalar, and theta^'s next stage input is stored as well (ps_col_adj_kernel with a PsAdjScalar).
// With a tangent (the flow's alone) the pack ends in a PsKeepTangent, and dw^'s next stage input is stored as well (ps_col_adj_kernel with a PsAdjSecond).
// TANGENT (a PsTangent first in the pack, where a PsScalar would be; with one only in the TANSC form below, never with a PsKeep): after the vorticity's work on a tile the
// same text runs once more on the perturbation dw^: Ph's second field, dw^ / dA with the VORTICITY's factors (hdrag and the LINEAR complex ones
// included) and mask, dg^ where the vorticity adds g^ (also under an unforced base, whose own arithmetic stays the unforced kernel's), no kick
// and no step count of its own, then its velocity and gradient as G fields 4-7 with zero means.  The vorticity's arithmetic is untouched.
// TANSC (a PsScalar, a PsTangent and a PsTangentScalar, in that order; never with a PsKeep or a PsTangents): the tangent of the system with a
// scalar.  Four passes per tile: the vorticity, the scalar, the TG text on dw^ (Ph field 2, G fields 6-9) and the TH text with TG on dtheta^ /
// dA_theta: Ph field 3, E_theta and the mask that keeps (0, 0), no g^, no dg^, no kick, zero means, i kx dtheta^, i ky dtheta^ to G fields 10, 11.
// TANGENTS (a PsTangents in the PsTangent's place; never with a PsScalar or a PsKeep): the TG text runs K times in a run-time loop, turn k on
// dW + k kstride / dA + k kstride, Ph field 1+k and G fields 4+4k .. 7+4k, with no dg^.  The text sees member k under the names it has for
// the one tangent (Ph, G and tg are shadowed by member k's in the loop's scope), so it is the same text and member k's bits are the TANGENT kernel's.
// TANSCS (a PsScalar, a PsTangents and a PsTangentsScalar, in that order; never with a PsKeep or a PsTangent): K tangent pairs on the system with a
// scalar.  The vorticity's pass, the scalar's, then a run-time loop whose turn k runs the two tangent passes of the TANSC form on member k: Ph,
// G, tg, dTh, dAt and TANSC itself are shadowed in the loop's scope (Ph fields 2+2k, 3+2k; G fields 6+6k .. 11+6k; dW, dA, dT, dAt + k kstride),
// so the text is that form's and member k's bits are the TANSC kernel's with dg^ = NULL.
template <int N, int S, bool FORCED = false, bool SCALAR = false, typename... Sc>
__global__ __launch_bounds__(kT) void ps_col_kernel(const float2* __restrict__ Ph, float2* __restrict__ G, float2* __restrict__ W,
                                                    float2* __restrict__ A, const float* __restrict__ mean, PsArgs a, int emit,
                                                    std::conditional_t<FORCED, PsForce, PsNoForce> fc, Sc... sc) {
    static_assert(!FORCED || S >= 1, "stage 0 only prepares: it has no forced form");
    constexpr bool STOCH = (std::is_same_v<Sc, PsStoch> || ... || false);
    constexpr bool LINEAR = (std::is_same_v<Sc, PsLinear> || ... || false);
    constexpr bool TANGENT = (std::is_same_v<Sc, PsTangent> || ... || false);
    constexpr bool TANGENTS = (std::is_same_v<Sc, PsTangents> || ... || false);
    constexpr bool TANSC = (std::is_same_v<Sc, PsTangentScalar> || ... || false);
    constexpr bool TANSCS = (std::is_same_v<Sc, PsTangentsScalar> || ... || false);
    constexpr bool KEEP_W = (std::is_same_v<Sc, PsKeep> || ... || false), KEEP_WT = (std::is_same_v<Sc, PsKeepScalar> || ... || false);
    constexpr bool KEEP_WD = (std::is_same_v<Sc, PsKeepTangent> || ... || false);
    constexpr bool STAGES = KEEP_W || KEEP_WT || KEEP_WD;
    static_assert(sizeof...(Sc) == (SCALAR ? 1 : 0) + (TANGENT ? 1 : 0) + (TANGENTS ? 1 : 0) + (TANSC ? 1 : 0) + (TANSCS ? 1 : 0) + (STOCH ? 1 : 0) + (LINEAR ? 1 : 0) + (STAGES ? 1 : 0),
                  "PsScalar is the SCALAR kernel's argument (PsTangent the TANGENT kernel's), PsLinear after it the LINEAR kernel's, PsStoch or the PsKeep last");
    static_assert(!TANGENT || (SCALAR == TANSC && (!STAGES || (KEEP_WD && !SCALAR))), "the tangent of the scalar system takes a PsScalar, a PsTangent and a PsTangentScalar; only the flow's tangent is recomputed with a stage store, a PsKeepTangent's");
    static_assert(!KEEP_WD || TANGENT, "the PsKeepTangent is the TANGENT kernels' stage store");
    static_assert(!TANSC || (SCALAR && TANGENT), "the PsTangentScalar follows a PsScalar and a PsTangent");
    static_assert(!TANGENTS || (SCALAR == TANSCS && !STAGES && !TANGENT), "K tangents: as the one tangent, and never beside it; with a scalar a PsTangentsScalar follows");
    static_assert(!TANSCS || (SCALAR && TANGENTS), "the PsTangentsScalar follows a PsScalar and a PsTangents");
    static_assert(!STAGES || (S >= 1 && S <= 3 && KEEP_WT == SCALAR && !STOCH),
                  "the stage store is that of stages 1-3 of the steady and the linear forms: a PsKeep (with a tangent: a PsKeepTangent) without a scalar, a PsKeepScalar with one");
    static_assert(!LINEAR || (FORCED && S >= 1 && S <= 3), "the complex factors are those of stages 1-3 of the forced form");
    static_assert(!STOCH || (FORCED && (S == 1 || S == 4)), "the kick is stage 4's and the step count stage 1's, both of the forced form");
    using L = PsLds<N>;
    constexpr int TPF = L::TPF, CW = L::LINES, RPI = kT / CW;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const cf* tab = ps_tables<N>(smem);
    unsigned char* lines = smem + L::TAB_BYTES;
    const int my1 = a.my1;
    const long ntiles = (a.nlines + CW - 1) / CW;
    const float dt = a.dt, dt2 = 0.5f * dt, dt3 = dt / 3.f, dt6 = dt / 6.f;
    [[maybe_unused]] float2* Th = nullptr;
    [[maybe_unused]] float2* At = nullptr;
    [[maybe_unused]] float hkdt = 0.f;
    if constexpr (SCALAR) {
        const PsScalar ps = pick<PsScalar>(sc...);
        Th = ps.T; At = ps.At; hkdt = ps.hkdt;
    }
    [[maybe_unused]] const float* samp = nullptr;
    [[maybe_unused]] const int* sids = nullptr;
    [[maybe_unused]] unsigned sk0 = 0, sk1 = 0, sn0 = 0, sn1 = 0;
    [[maybe_unused]] float sqdt = 0.f;
    if constexpr (STOCH) {
        const PsStoch st = pick<PsStoch>(sc...);
        if constexpr (S == 1) {
            if (blockIdx.x == 0 && threadIdx.x == 0) *st.clock = *st.clock + 1;      // no workgroup of this launch reads it
        } else {
            const unsigned long long n = (unsigned long long)(*st.clock - 1);        // this step's index: stage 1 has counted it
            samp = st.amp; sids = st.ids; sk0 = st.k0; sk1 = st.k1; sqdt = st.sqdt;
            sn0 = (unsigned)n; sn1 = (unsigned)(n >> 32);
        }
    }
    [[maybe_unused]] const float2* lin = nullptr;
    if constexpr (LINEAR) lin = pick<PsLinear>(sc...).lin;
    [[maybe_unused]] PsTangent tg{};
    if constexpr (TANGENT) tg = pick<PsTangent>(sc...);
    [[maybe_unused]] float2* dTh = nullptr;
    [[maybe_unused]] float2* dAt = nullptr;
    if constexpr (TANSC) {
        const PsTangentScalar tt = pick<PsTangentScalar>(sc...);
        dTh = tt.dT; dAt = tt.dAt;
    }
    [[maybe_unused]] float2* stage_out = nullptr;
    [[maybe_unused]] float2* tstage_out = nullptr;
    if constexpr (KEEP_W) stage_out = pick<PsKeep>(sc...).stage;
    if constexpr (KEEP_WT) {
        const PsKeepScalar ke = pick<PsKeepScalar>(sc...);
        stage_out = ke.stage; tstage_out = ke.tstage;
    }
    [[maybe_unused]] float2* dstage_out = nullptr;
    if constexpr (KEEP_WD) {
        const PsKeepTangent ke = pick<PsKeepTangent>(sc...);
        stage_out = ke.stage; dstage_out = ke.dstage;
    }
    for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int tx = threadIdx.x;
        asm volatile("" : "+v"(tx));
#include "pspec_col_tile.inc"
        [[maybe_unused]] size_t gbase = 0;
        [[maybe_unused]] bool gok = false;
        if constexpr (FORCED) {
            gbase = fc.shared ? (size_t)lj * N : wbase;
            gok = lok && fc.g != nullptr;
        }
        [[maybe_unused]] unsigned sid = 0;
        if constexpr (STOCH && S == 4) sid = lok ? (unsigned)sids[lb] : 0u;
        int tv = tid;
        asm volatile("" : "+v"(tv));
        const float ky = a.ky1 * (float)lj;
        [[maybe_unused]] size_t dgbase = 0;
        [[maybe_unused]] bool dgok = false;
        if constexpr (TANGENT) {
            dgbase = tg.dshared ? (size_t)lj * N : wbase;
            dgok = lok && tg.dg != nullptr;
        }
        // one field through the tile, as plain text per field (the note in pspec_col_pass.inc): first the vorticity, then the scalar or the tangent
        {
            constexpr bool TH = false, TG = false;
#include "pspec_col_pass.inc"
        }
        if constexpr (SCALAR) {
            constexpr bool TH = true, TG = false;
#include "pspec_col_pass.inc"
        }
        if constexpr (TANGENT) {
            constexpr bool TH = false, TG = true;
#include "pspec_col_pass.inc"
        }
        if constexpr (TANSC) {
            constexpr bool TH = true, TG = true;
#include "pspec_col_pass.inc"
        }
        if constexpr (TANSCS) {
            const PsTangents ts = pick<PsTangents>(sc...);
            const PsTangentsScalar tu = pick<PsTangentsScalar>(sc...);
            const float2* const Ph0 = Ph;
            float2* const G0 = G;
            for (int k = 0; k < ts.K; ++k) {            // member k's pair under the names of the TANSC form: its two passes, in its text
                constexpr bool TANSC = true;
                const float2* Ph = Ph0 + (size_t)(2 * k) * a.fstride;
                float2* G = G0 + (size_t)(6 * k) * a.fstride;
                const PsTangent tg{ts.dW + (size_t)k * ts.kstride, ts.dA + (size_t)k * ts.kstride, nullptr, 0};
                float2* const dTh = tu.dT + (size_t)k * ts.kstride;
                float2* const dAt = tu.dAt + (size_t)k * ts.kstride;
                {
                    constexpr bool TH = false, TG = true;
#include "pspec_col_pass.inc"
                }
                {
                    constexpr bool TH = true, TG = true;
#include "pspec_col_pass.inc"
                }
            }
        }
        if constexpr (TANGENTS && !TANSCS) {
            const PsTangents ts = pick<PsTangents>(sc...);
            const float2* const Ph0 = Ph;
            float2* const G0 = G;
            for (int k = 0; k < ts.K; ++k) {            // member k under the one tangent's names
                const float2* Ph = Ph0 + (size_t)k * a.fstride;
                float2* G = G0 + (size_t)(4 * k) * a.fstride;
                const PsTangent tg{ts.dW + (size_t)k * ts.kstride, ts.dA + (size_t)k * ts.kstride, nullptr, 0};
                constexpr bool TH = false, TG = true;
#include "pspec_col_pass.inc"
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------- reverse mode (restatement: tests/pspec_adjoint_oracle.py)
// The vector-Jacobian product of the forced step.  Cotangents are real band-limited fields paired by the grid sum, kept as spectra in the
// layout of W, so E and the mask are their own adjoints.  With kappa the cotangent of a stage's N and s that stage's state,
//     N'(s)^T kappa = M [u kappa_x + v kappa_y] - M [kappa_x w_y - kappa_y w_x]^ / |k|^2       (u, v, w_x, w_y of s; the means in u, v)
// ps_row_adj_kernel is the SCALAR row kernel's twin: three inverse transforms along y (u + i v and w_x + i w_y from G fields 0-3 of s,
// kappa_x + i kappa_y from G fields 4 and 5), the two products in registers, two forward transforms, the kept modes to Ph fields 0 and 1.  Two
// complex lines are live at a time, as there.
// SCALAR (a PsAdjGrad is then the last argument; restatement: tests/pspec_scalar_adjoint_oracle.py).  With mu the cotangent of a stage's N_theta beside kappa, that of its N_w:
//     r_w     = M [u kappa_x + v kappa_y]^ - M [kappa_x w_y - kappa_y w_x + mu_x (theta_y + Gy) - mu_y (theta_x + Gx)]^ / |k|^2
//     r_theta = M_theta [u mu_x + v mu_y - by kappa_x + bx kappa_y]^
// Five inverse transforms along y (G fields 0-3: u, v, w_x, w_y; 4, 5: grad kappa; 6, 7: grad theta; 8, 9: grad mu), three products, three
// forward transforms, the kept modes to Ph fields 0 (u . grad kappa), 1 (the sum the inverse Laplacian takes) and 2 (the scalar's).  The
// buoyancy's adjoint is linear in grad kappa, which the row holds in physical space: two fused multiply-adds, no transform; b = 0 is the
// passive scalar's.  Three complex lines are live at a time: u, grad kappa and grad mu while the first and the third product leave, then the
// line of u takes grad w and that of grad kappa takes grad theta.
template <int N, bool SCALAR = false, typename... Gr>
__global__ __launch_bounds__(kT) void ps_row_adj_kernel(const float2* __restrict__ G, float2* __restrict__ Ph, PsArgs a, Gr... grad) {
    static_assert(sizeof...(Gr) == (SCALAR ? 1 : 0), "the PsAdjGrad is the SCALAR kernel's argument");
    using L = PsLds<N>;
    constexpr int TPF = L::TPF;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const cf* tab = ps_tables<N>(smem);
    unsigned char* lines = smem + L::TAB_BYTES;
    const int my1 = a.my1;
    const long niter = (a.nlines + L::LINES - 1) / L::LINES;
    for (long it = blockIdx.x; it < niter; it += gridDim.x) {
#include "pspec_row_line.inc"
        cf zu[16], zk[16];
        ps_row_load2<N>(g0, g0 + a.fstride, tid, my1, zu);                           // u + i v
        fft_line<float, N, true>(zu, tab, tab + N / 2, xb, tid);
        __builtin_amdgcn_sched_barrier(0);
        ps_row_load2<N>(g0 + 4 * a.fstride, g0 + 5 * a.fstride, tid, my1, zk);       // kappa_x + i kappa_y: stays
        fft_line<float, N, true>(zk, tab, tab + N / 2, xb, tid);
        if constexpr (!SCALAR) {
#pragma unroll
            for (int m = 0; m < 16; ++m) zu[m] = {zu[m].x * zk[m].x + zu[m].y * zk[m].y, 0.f};    // u kappa_x + v kappa_y
            __builtin_amdgcn_sched_barrier(0);
            fft_line<float, N, false>(zu, tab, tab + N / 2, xb, tid);
            ps_row_store<N>(zu, Ph + (size_t)row * my1, tid, my1, valid);
            __builtin_amdgcn_sched_barrier(0);
            ps_row_load2<N>(g0 + 2 * a.fstride, g0 + 3 * a.fstride, tid, my1, zu);   // w_x + i w_y
            fft_line<float, N, true>(zu, tab, tab + N / 2, xb, tid);
#pragma unroll
            for (int m = 0; m < 16; ++m) zu[m] = {zk[m].x * zu[m].y - zk[m].y * zu[m].x, 0.f};    // kappa_x w_y - kappa_y w_x
            __builtin_amdgcn_sched_barrier(0);
        } else {
            const PsAdjGrad gr = pick<PsAdjGrad>(grad...);
            cf zm[16];
#pragma unroll
            for (int m = 0; m < 16; ++m) zm[m] = {zu[m].x * zk[m].x + zu[m].y * zk[m].y, 0.f};    // u kappa_x + v kappa_y: u, v stay
            __builtin_amdgcn_sched_barrier(0);
            fft_line<float, N, false>(zm, tab, tab + N / 2, xb, tid);
            ps_row_store<N>(zm, Ph + (size_t)row * my1, tid, my1, valid);
            __builtin_amdgcn_sched_barrier(0);
            ps_row_load2<N>(g0 + 8 * a.fstride, g0 + 9 * a.fstride, tid, my1, zm);   // mu_x + i mu_y: stays
            fft_line<float, N, true>(zm, tab, tab + N / 2, xb, tid);
#pragma unroll
            for (int m = 0; m < 16; ++m)                                             // u mu_x + v mu_y - by kappa_x + bx kappa_y
                zu[m] = {fmaf(zu[m].x, zm[m].x, fmaf(zu[m].y, zm[m].y, fmaf(-gr.by, zk[m].x, gr.bx * zk[m].y))), 0.f};
            __builtin_amdgcn_sched_barrier(0);
            fft_line<float, N, false>(zu, tab, tab + N / 2, xb, tid);
            ps_row_store<N>(zu, Ph + 2 * a.fstride + (size_t)row * my1, tid, my1, valid);
            __builtin_amdgcn_sched_barrier(0);
            ps_row_load2<N>(g0 + 2 * a.fstride, g0 + 3 * a.fstride, tid, my1, zu);   // w_x + i w_y
            fft_line<float, N, true>(zu, tab, tab + N / 2, xb, tid);
#pragma unroll
            for (int m = 0; m < 16; ++m) zu[m] = {zk[m].x * zu[m].y - zk[m].y * zu[m].x, 0.f};    // kappa_x w_y - kappa_y w_x
            __builtin_amdgcn_sched_barrier(0);
            ps_row_load2<N>(g0 + 6 * a.fstride, g0 + 7 * a.fstride, tid, my1, zk);   // theta_x + i theta_y
            fft_line<float, N, true>(zk, tab, tab + N / 2, xb, tid);
#pragma unroll
            for (int m = 0; m < 16; ++m)                                             // + mu_x (theta_y + Gy) - mu_y (theta_x + Gx)
                zu[m].x = fmaf(zm[m].x, zk[m].y + gr.gy, fmaf(-zm[m].y, zk[m].x + gr.gx, zu[m].x));
            __builtin_amdgcn_sched_barrier(0);
        }
        fft_line<float, N, false>(zu, tab, tab + N / 2, xb, tid);
        ps_row_store<N>(zu, Ph + a.fstride + (size_t)row * my1, tid, my1, valid);
    }
}

// The row pass of the second-order adjoint (nns_spec_ns_step_second_adjoint_f32; restatement: tests/pspec_second_adjoint_oracle.py):
// ps_row_adj_kernel's twin, as ps_row_tan_kernel is ps_row_kernel's.  G fields 0-3 are the state's (u, v, w_x, w_y, the means in u, v), 4 and 5
// grad kappa, 6-9 the tangent stage's (du, dv, dw_x, dw_y: no mean flow), 10 and 11 grad dkappa.  Ph fields 0 and 1 take
//     q1 = u kappa_x + v kappa_y     and     q2 = kappa_x w_y - kappa_y w_x,
// spelt with ps_row_adj_kernel's expressions from the same transforms of the same G fields, so the first-order cotangents stay bitwise the
// adjoint's; 2 and 3 their derivatives in the direction,
//     dq1 = u dkappa_x + v dkappa_y + du kappa_x + dv kappa_y     and     dq2 = dkappa_x w_y - dkappa_y w_x + kappa_x dw_y - kappa_y dw_x.
// Six inverse transforms, each line read and transformed once, and FOUR forward ones, one per product: packing q + i dq into one forward
// transform would need the mirrored mode of another lane to take the pair apart again, an exchange the row pass does not have.
// The order taken: u + i v and grad kappa, q1 out; grad dkappa, whose product with u (16 reals, zp) frees the line of u; grad w into that line,
// which gives q2 and, with grad dkappa, 16 more reals (zq), q2 out; du + i dv closes dq1, grad dw closes dq2.  grad kappa stays throughout.
// Each product of dq1 and dq2 has no line in common with the other, so one of them waits as 16 reals while the other's lines come in: three
// complex lines are live but for the transform of grad w, which runs beside grad kappa, grad dkappa and zp (three and a half, as in
// ps_row_tans_kernel); holding to three there would take a seventh inverse transform (grad dkappa twice).  The lane's index is pinned anew before
// each of the three later pairs of transforms (tb, tc, td), as ps_row_tans_kernel pins it per turn: what six loads, ten transforms and four stores
// derive from it (element offsets, predicates, twiddle addresses) is otherwise computed once and held across the whole row.
template <int N>
__global__ __launch_bounds__(kT) void ps_row_adj2_kernel(const float2* __restrict__ G, float2* __restrict__ Ph, PsArgs a) {
    using L = PsLds<N>;
    constexpr int TPF = L::TPF;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const cf* tab = ps_tables<N>(smem);
    unsigned char* lines = smem + L::TAB_BYTES;
    const int my1 = a.my1;
    const long niter = (a.nlines + L::LINES - 1) / L::LINES;
    for (long it = blockIdx.x; it < niter; it += gridDim.x) {
#include "pspec_row_line.inc"
        cf zu[16], zk[16], zd[16];
        float zp[16], zq[16];
        ps_row_load2<N>(g0, g0 + a.fstride, tid, my1, zu);                           // u + i v
        fft_line<float, N, true>(zu, tab, tab + N / 2, xb, tid);
        __builtin_amdgcn_sched_barrier(0);
        ps_row_load2<N>(g0 + 4 * a.fstride, g0 + 5 * a.fstride, tid, my1, zk);       // kappa_x + i kappa_y: stays
        fft_line<float, N, true>(zk, tab, tab + N / 2, xb, tid);
#pragma unroll
        for (int m = 0; m < 16; ++m) zd[m] = {zu[m].x * zk[m].x + zu[m].y * zk[m].y, 0.f};        // u kappa_x + v kappa_y: u, v stay
        __builtin_amdgcn_sched_barrier(0);
        fft_line<float, N, false>(zd, tab, tab + N / 2, xb, tid);
        ps_row_store<N>(zd, Ph + (size_t)row * my1, tid, my1, valid);
        int tb = tid;
        asm volatile("" : "+v"(tb));
        __builtin_amdgcn_sched_barrier(0);
        ps_row_load2<N>(g0 + 10 * a.fstride, g0 + 11 * a.fstride, tb, my1, zd);     // dkappa_x + i dkappa_y: stays until grad w has met it
        fft_line<float, N, true>(zd, tab, tab + N / 2, xb, tb);
#pragma unroll
        for (int m = 0; m < 16; ++m) zp[m] = zu[m].x * zd[m].x + zu[m].y * zd[m].y;               // u dkappa_x + v dkappa_y: u, v leave
        __builtin_amdgcn_sched_barrier(0);
        ps_row_load2<N>(g0 + 2 * a.fstride, g0 + 3 * a.fstride, tb, my1, zu);       // w_x + i w_y
        fft_line<float, N, true>(zu, tab, tab + N / 2, xb, tb);
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            zq[m] = zd[m].x * zu[m].y - zd[m].y * zu[m].x;                                        // dkappa_x w_y - dkappa_y w_x: dkappa leaves
            zu[m] = {zk[m].x * zu[m].y - zk[m].y * zu[m].x, 0.f};                                 // kappa_x w_y - kappa_y w_x
        }
        __builtin_amdgcn_sched_barrier(0);
        fft_line<float, N, false>(zu, tab, tab + N / 2, xb, tb);
        ps_row_store<N>(zu, Ph + a.fstride + (size_t)row * my1, tb, my1, valid);
        int tc = tid;
        asm volatile("" : "+v"(tc));
        __builtin_amdgcn_sched_barrier(0);
        ps_row_load2<N>(g0 + 6 * a.fstride, g0 + 7 * a.fstride, tc, my1, zu);       // du + i dv
        fft_line<float, N, true>(zu, tab, tab + N / 2, xb, tc);
#pragma unroll
        for (int m = 0; m < 16; ++m) zu[m] = {fmaf(zu[m].x, zk[m].x, fmaf(zu[m].y, zk[m].y, zp[m])), 0.f};     // + du kappa_x + dv kappa_y
        __builtin_amdgcn_sched_barrier(0);
        fft_line<float, N, false>(zu, tab, tab + N / 2, xb, tc);
        ps_row_store<N>(zu, Ph + 2 * a.fstride + (size_t)row * my1, tc, my1, valid);
        int td = tid;
        asm volatile("" : "+v"(td));
        __builtin_amdgcn_sched_barrier(0);
        ps_row_load2<N>(g0 + 8 * a.fstride, g0 + 9 * a.fstride, td, my1, zu);       // dw_x + i dw_y
        fft_line<float, N, true>(zu, tab, tab + N / 2, xb, td);
#pragma unroll
        for (int m = 0; m < 16; ++m) zu[m] = {fmaf(zk[m].x, zu[m].y, fmaf(-zk[m].y, zu[m].x, zq[m])), 0.f};    // + kappa_x dw_y - kappa_y dw_x
        __builtin_amdgcn_sched_barrier(0);
        fft_line<float, N, false>(zu, tab, tab + N / 2, xb, td);
        ps_row_store<N>(zu, Ph + 3 * a.fstride + (size_t)row * my1, td, my1, valid);
    }
}

// The adjoint column pass, S = 4 .. 0 in the order it runs (ps_col_kernel's tile: pspec_col_tile.inc, pspec_stage.inc).  With lam the cotangent of the step's
// result, r = N'(s)^T kappa of the stage just evaluated by the row pass (S < 4: Ph fields 0 and 1 staged and forward-transformed along x,
// r = keep ? Q1 - Q2 / |k|^2 : 0) and E - 1, E^2 - 1 in the forward's expm1 form:
//     S = 4                                    kappa4 = dt/6 lam                      prepares s3
//     S = 3   wbar  = E^2 lam + E^2 r          kappa3 = dt/3 E lam + dt E r           prepares s2
//     S = 2   wbar += E r                      kappa2 = dt/3 E lam + dt/2 r           prepares s1
//     S = 1   wbar += E r                      kappa1 = dt/6 E^2 lam + dt/2 E r       prepares s0
//     S = 0   lam   = wbar + r                 (the cotangent of the step's input, the lam of the step before)
// gbar += kappa in every stage that makes one.  lam, wbar and gbar are lane-owned and coalesced, like W / A.  Preparing: the four spectra of
// the state (ad.state, the forward's field<0..3>: pspec_field.inc, the mean in the (0, 0) mode) inverse-transformed along x to G fields 0-3, and
// i kx kappa^, i ky kappa^ to G fields 4 and 5 (these first: kappa's registers are free before the state is loaded).
// With a PsAdjScalar (the scalar and the buoyant step; restatement: tests/pspec_scalar_adjoint_oracle.py) the same sequence runs on the scalar
// after the vorticity's work on a tile (pspec_col_adj_pass.inc holds the recurrences, included once per spectrum), with
// E_theta = exp(-kappa |k|^2 dt / 2) and mu, m, thetabar where the vorticity has E, lam, kappa, wbar:
//     S = 4                                             m4 = dt/6 mu
//     S = 3   thetabar  = E_theta^2 (mu + r_theta)      m3 = dt/3 E_theta mu + dt E_theta r_theta
//     S = 2   thetabar += E_theta r_theta               m2 = dt/3 E_theta mu + dt/2 r_theta
//     S = 1   thetabar += E_theta r_theta               m1 = dt/6 E_theta^2 mu + dt/2 E_theta r_theta
//     S = 0   mu        = thetabar + r_theta
// r_w takes Ph fields 0 and 1 as without the scalar (field 1 now also holds the scalar's share), r_theta = keep_theta ? Ph field 2 : 0.
// Preparing: i kx kappa^, i ky kappa^ to G fields 4 and 5 and i kx m^, i ky m^ to 8 and 9 (each while its registers are still there), then the
// state's four spectra to G fields 0-3 and i kx theta^, i ky theta^ of the state's scalar to 6 and 7.  One spectrum's registers at a time.
// LINEAR (a PsAdjLinear / PsAdjScalarLinear; S = 3, 2, 1; restatement: tests/pspec_linear_adjoint_oracle.py): the forward's factor is the complex
// E_k = exp(lambda_k dt / 2) with E(-k) = conj(E(k)), so it maps spectra of real fields to such, and under the grid sum's pairing
// sum_k Re(conj(a_k) E_k b_k) = sum_k Re(conj(conj(E_k) a_k) b_k): the transpose multiplies by conj(E_k).  The recurrences above hold as they stand
// with conj(E) - 1 and conj(E^2) - 1 for the vorticity: the forward's 8-byte load and ps_linear_factors, the imaginary parts negated.  The
// scalar's E_theta stays real, and the row adjoint is untouched (beta sits in lambda, not in N).  The white-in-time kick is added to w^ after the
// step and does not depend on the state: its Jacobian is the identity, the saved start spectra already carry it, and there is nothing to transpose.
// OPERATOR (a PsAdjOperator / PsAdjScalarOperator; S = 3, 2, 1; restatement: tests/pspec_operator_grad_oracle.py): the LINEAR kernel that also
// sums the cotangent of the table l = lambda dt / 2.  With E = exp(l), d s1 / dl = s1, d s2 / dl = E w0, d s3 / dl = s3 + E^2 w0 and
// d w1 / dl = (s3 + E^2 w0) / 3 + 2/3 E (s1 + s2) -- no N and no division by E, so a stiff mode is safe -- and a cotangent c of z = D dl gives
// c conj(D).  r of stage S is the cotangent of s_S and lam that of w1, so per mode
//     S = 3   lstep  = (r + lam / 3) (conj(s3) + conj(E^2) conj(w0))
//     S = 2   lstep += conj(E) (r conj(w0) + 2/3 lam conj(s2))
//     S = 1   lbar  += lstep + (r + 2/3 conj(E) lam) conj(s1)               (= on the call's first step: ginit)
// before stage 0 overwrites lam: ad.own is s_S and ad.w0 the step's start, five more reads of a compact field per step and three reads and
// three writes of the two sums.  A step's sum is made on its own (lstep, a field of the workspace that is idle in these stages) and then
// added, so nsteps steps in one call are bitwise the sum of nsteps calls of one step.  Both are lane-owned like gbar: no atomics, and a grid's
// sum does not depend on its batch neighbours.  The weight of a stored mode, 1 / n
// and the symmetry of the ky = 0 line are the caller's (nns.h: nns_spec_ns_step_operator_adjoint_f32).
// SECOND (a PsAdjSecond, or for stages 3-1 of a linear step a PsAdjSecondLinear; restatement: tests/pspec_second_adjoint_oracle.py): after the
// vorticity's work on a tile the same text runs once more (TD) on the derivative in the direction: dlam, dkappa, dwbar, dgbar where the first pass
// has lam, kappa, wbar, gbar, dr = keep ? DQ1 - DQ2 / |k|^2 : 0 from Ph fields 2 and 3, the vorticity's factors (conj(E) from the table in the
// LINEAR form) and mask, i kx dkappa^, i ky dkappa^ to G fields 10 and 11.  Then the state's four spectra to G fields 0-3 as ever and the tangent
// stage's (ad.dstate) to G fields 6-9 with zero in the (0, 0) mode.  The first pass is the adjoint's own, so lam, wbar and gbar are its bits.
template <int N, int S, typename Ad>
__global__ __launch_bounds__(kT) void ps_col_adj_kernel(const float2* __restrict__ Ph, float2* __restrict__ G, const float* __restrict__ mean,
                                                        PsArgs a, Ad ad) {
    static_assert(S >= 0 && S <= 4, "adjoint stages 4 .. 0");
    constexpr bool OPERATOR = std::is_same_v<Ad, PsAdjOperator> || std::is_same_v<Ad, PsAdjScalarOperator>;
    constexpr bool SCALAR = std::is_same_v<Ad, PsAdjScalar> || std::is_same_v<Ad, PsAdjScalarLinear> || std::is_same_v<Ad, PsAdjScalarOperator>;
    constexpr bool SECOND = std::is_same_v<Ad, PsAdjSecond> || std::is_same_v<Ad, PsAdjSecondLinear>;
    constexpr bool LINEAR = std::is_same_v<Ad, PsAdjLinear> || std::is_same_v<Ad, PsAdjScalarLinear> || OPERATOR || std::is_same_v<Ad, PsAdjSecondLinear>;
    static_assert(SCALAR || SECOND || std::is_same_v<Ad, PsAdj> || std::is_same_v<Ad, PsAdjLinear> || std::is_same_v<Ad, PsAdjOperator>,
                  "a PsAdj, or a PsAdjScalar for the step with a scalar; their LINEAR forms for a linear step, their OPERATOR forms for the table's cotangent; a PsAdjSecond or its LINEAR form for the second-order adjoint");
    static_assert(!LINEAR || (S >= 1 && S <= 3), "the conjugate factors are those of adjoint stages 3-1: stages 4 and 0 apply none");
    using L = PsLds<N>;
    constexpr int TPF = L::TPF, CW = L::LINES, RPI = kT / CW;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const cf* tab = ps_tables<N>(smem);
    unsigned char* lines = smem + L::TAB_BYTES;
    const int my1 = a.my1;
    const long ntiles = (a.nlines + CW - 1) / CW;
    [[maybe_unused]] const float dt = a.dt, dt2 = 0.5f * dt, dt3 = dt / 3.f, dt6 = dt / 6.f;
    for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int tx = threadIdx.x;
        asm volatile("" : "+v"(tx));
#include "pspec_col_tile.inc"
        int tv = tid;
        asm volatile("" : "+v"(tv));
        const float ky = a.ky1 * (float)lj;
        // Ph's field `ph` of the tile through the LDS transpose, forward-transformed along x
        [[maybe_unused]] auto consume = [&](const float2* ph, cf (&z)[16]) {
#include "pspec_stage.inc"
        };
        [[maybe_unused]] const float U0 = S >= 1 && lok ? mean[2 * lb] : 0.f, V0 = S >= 1 && lok ? mean[2 * lb + 1] : 0.f;
        // field F of the spectrum y, transformed along x and written to G through the LDS transpose: ps_col_kernel's, without its pin of y
        [[maybe_unused]] auto field = [&](auto fc, const cf (&y)[16]) {
            constexpr int F = decltype(fc)::value, FK = F;
            int te = tv;
            asm volatile("" : "+v"(te));
#include "pspec_field.inc"
        };
        {
            constexpr bool TH = false, TD = false;
#include "pspec_col_adj_pass.inc"
        }
        if constexpr (SCALAR) {
            constexpr bool TH = true, TD = false;
#include "pspec_col_adj_pass.inc"
        }
        if constexpr (SECOND) {
            constexpr bool TH = false, TD = true;
#include "pspec_col_adj_pass.inc"
        }
        if constexpr (S >= 1) {
            cf y[16];
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                const float2 w = lok ? ad.state[wbase + tv + TPF * m] : make_float2(0.f, 0.f);
                y[m] = {w.x, w.y};
            }
            static_for<0, 4>([&](auto fc) { field(fc, y); });
            if constexpr (SECOND) {                     // the tangent stage's four spectra, as ps_col_kernel's tangent pass emits them: no mean flow
#pragma unroll
                for (int m = 0; m < 16; ++m) {
                    const float2 w = lok ? ad.dstate[wbase + tv + TPF * m] : make_float2(0.f, 0.f);
                    y[m] = {w.x, w.y};
                }
                static_for<6, 10>([&](auto fc) {
                    constexpr int F = decltype(fc)::value, FK = F - 6;
                    constexpr float U0 = 0.f, V0 = 0.f;
                    int te = tv;
                    asm volatile("" : "+v"(te));
#include "pspec_field.inc"
                });
            }
            if constexpr (SCALAR) {
#pragma unroll
                for (int m = 0; m < 16; ++m) {
                    const float2 w = lok ? ad.tstate[wbase + tv + TPF * m] : make_float2(0.f, 0.f);
                    y[m] = {w.x, w.y};
                }
                static_for<6, 8>([&](auto fc) { field(fc, y); });
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------- init / output (pointwise)
// W[b][j][i] = M (i kx v^ - i ky u^)   from rfft2 spectra uh, vh [B][nx][nh]; mean[b] = (u^(0,0), v^(0,0)) / (nx ny)
__global__ void ps_init_kernel(const float2* __restrict__ uh, const float2* __restrict__ vh, float2* __restrict__ W, float* __restrict__ mean,
                               int batch, int nx, int ny, int my1, float kx1, float ky1, float inv_n) {
    const long total = (long)batch * my1 * nx, nh = ny / 2 + 1;
    for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
        const int i = (int)(q % nx), j = (int)((q / nx) % my1);
        const long b = q / ((long)nx * my1);
        const int mx = i < nx / 2 ? i : i - nx;
        const size_t s = ((size_t)b * nx + i) * nh + j;
        const float2 u = uh[s], v = vh[s];
        const bool keep = 3 * (mx < 0 ? -mx : mx) < nx && (mx | j) != 0;
        const float kx = kx1 * (float)mx, ky = ky1 * (float)j;
        // i kx v - i ky u = (-(kx v.y - ky u.y), kx v.x - ky u.x)
        W[q] = keep ? make_float2(ky * u.y - kx * v.y, kx * v.x - ky * u.x) : make_float2(0.f, 0.f);
        if (i == 0 && j == 0) { mean[2 * b] = u.x * inv_n; mean[2 * b + 1] = v.x * inv_n; }
    }
}

// rfft2 spectra of u_x, u_y, v_x, v_y, u, v ([6][B][nx][nh]) from W and the means
__global__ void ps_derivs_kernel(const float2* __restrict__ W, const float* __restrict__ mean, float2* __restrict__ out,
                                 int batch, int nx, int ny, int my1, float kx1, float ky1) {
    const long nh = ny / 2 + 1, per = (long)batch * nx * nh;
    for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < per; q += (long)gridDim.x * blockDim.x) {
        const int j = (int)(q % nh), i = (int)((q / nh) % nx);
        const long b = q / ((long)nx * nh);
        const int mx = i < nx / 2 ? i : i - nx;
        cf u = {0.f, 0.f}, v = {0.f, 0.f}, ux = u, uy = u, vx = u, vy = u;
        if (j < my1) {
            const float2 w2 = W[((size_t)b * my1 + j) * nx + i];
            const float kx = kx1 * (float)mx, ky = ky1 * (float)j, k2 = kx * kx + ky * ky;
            const cf psi = k2 > 0.f ? cf{w2.x / k2, w2.y / k2} : cf{0.f, 0.f};
            u = imul(ky, psi);
            v = imul(-kx, psi);
            ux = imul(kx, u); uy = imul(ky, u); vx = imul(kx, v); vy = imul(ky, v);
            if (i == 0 && j == 0) {
                const float n = (float)nx * (float)ny;
                u = {mean[2 * b] * n, 0.f}; v = {mean[2 * b + 1] * n, 0.f};
            }
        }
        const cf f[6] = {ux, uy, vx, vy, u, v};
#pragma unroll
        for (int k = 0; k < 6; ++k) out[k * per + q] = make_float2(f[k].x, f[k].y);
    }
}

// q = 2 rho (u_x v_y - u_y v_x) from d = [u_x, u_y, v_x, v_y] ([4][n])
__global__ void ps_source_kernel(const float* d, float* q, long n, float two_rho) {      // q may alias d's first field
    for (long k = blockIdx.x * (long)blockDim.x + threadIdx.x; k < n; k += (long)gridDim.x * blockDim.x)
        q[k] = two_rho * (d[k] * d[3 * n + k] - d[n + k] * d[2 * n + k]);
}

// p^ = -M q^ / |k|^2 in place (rfft2 layout)
__global__ void ps_pressure_kernel(float2* __restrict__ qh, int batch, int nx, int ny, float kx1, float ky1) {
    const long nh = ny / 2 + 1, per = (long)batch * nx * nh;
    for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < per; q += (long)gridDim.x * blockDim.x) {
        const int j = (int)(q % nh), i = (int)((q / nh) % nx);
        const int mx = i < nx / 2 ? i : i - nx;
        const bool keep = 3 * (mx < 0 ? -mx : mx) < nx && 3 * j < ny && (mx | j) != 0;
        const float kx = kx1 * (float)mx, ky = ky1 * (float)j, k2 = kx * kx + ky * ky;
        const float2 z = qh[q];
        qh[q] = keep ? make_float2(-z.x / k2, -z.y / k2) : make_float2(0.f, 0.f);
    }
}

// the same with buoyancy: p^ = -M (q^ + i (k . rho b) theta^) / |k|^2, theta^ read from the compact T [B][my1][nx] (keep implies j < my1)
__global__ void ps_pressure_buoyant_kernel(float2* __restrict__ qh, const float2* __restrict__ T, int batch, int nx, int ny, int my1, float kx1,
                                           float ky1, float rbx, float rby) {
    const long nh = ny / 2 + 1, per = (long)batch * nx * nh;
    for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < per; q += (long)gridDim.x * blockDim.x) {
        const int j = (int)(q % nh), i = (int)((q / nh) % nx);
        const long b = q / ((long)nx * nh);
        const int mx = i < nx / 2 ? i : i - nx;
        const bool keep = 3 * (mx < 0 ? -mx : mx) < nx && 3 * j < ny && (mx | j) != 0;
        const float kx = kx1 * (float)mx, ky = ky1 * (float)j, k2 = kx * kx + ky * ky;
        const float2 z = qh[q];
        float2 o = make_float2(0.f, 0.f);
        if (keep) {
            const float2 t = T[((size_t)b * my1 + j) * nx + i];
            const float kb = kx * rbx + ky * rby;
            o = make_float2(-(z.x - kb * t.y) / k2, -(z.y + kb * t.x) / k2);
        }
        qh[q] = o;
    }
}

// T[b][j][i] = M_theta th[b][i][j] from the rfft2 spectrum th [B][nx][nh]: the 2/3 rule, the (0, 0) mode kept
__global__ void ps_scalar_compact_kernel(const float2* __restrict__ th, float2* __restrict__ T, int batch, int nx, int ny, int my1) {
    const long total = (long)batch * my1 * nx, nh = ny / 2 + 1;
    for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
        const int i = (int)(q % nx), j = (int)((q / nx) % my1);
        const long b = q / ((long)nx * my1);
        const int mx = i < nx / 2 ? i : i - nx;
        T[q] = 3 * (mx < 0 ? -mx : mx) < nx ? th[((size_t)b * nx + i) * nh + j] : make_float2(0.f, 0.f);
    }
}

// the rfft2 spectrum th [B][nx][nh] of T: zero beyond the kept y-wavenumbers
__global__ void ps_scalar_expand_kernel(const float2* __restrict__ T, float2* __restrict__ th, int batch, int nx, int ny, int my1) {
    const long nh = ny / 2 + 1, per = (long)batch * nx * nh;
    for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < per; q += (long)gridDim.x * blockDim.x) {
        const int j = (int)(q % nh), i = (int)((q / nh) % nx);
        const long b = q / ((long)nx * nh);
        th[q] = j < my1 ? T[((size_t)b * my1 + j) * nx + i] : make_float2(0.f, 0.f);
    }
}

// ---------------------------------------------------------------------------------------------------- diagnostics
// out[b] = (E, Z, P): fluctuation energy 1/2 <|u - <u>|^2>, enstrophy 1/2 <w^2>, power input <f_s . u>, by Parseval over the stored half
// spectrum (weight 1 on the j = 0 line, 2 on j > 0), normalised by (nx ny)^2.  One workgroup per grid; every lane sums its strided
// elements in float64, then a wave64 shuffle tree and the waves' partials through LDS in index order: no atomics, so the sums repeat
// bitwise and a grid's numbers do not depend on its batch neighbours.
constexpr int kDiagT = 1024;

__global__ __launch_bounds__(kDiagT) void ps_diag_kernel(const float2* __restrict__ W, const float2* __restrict__ Gh, int gshared,
                                                          double* __restrict__ out, int nx, int my1, double kx1, double ky1, double inv_n2) {
    __shared__ double part[kDiagT / kWave][3];
    const long per = (long)my1 * nx;
    const float2* w = W + (size_t)blockIdx.x * per;
    const float2* g = Gh ? Gh + (gshared ? 0 : (size_t)blockIdx.x * per) : nullptr;
    double e = 0., z = 0., p = 0.;
    for (long q = threadIdx.x; q < per; q += kDiagT) {
        const int i = (int)(q % nx), j = (int)(q / nx);
        const int mx = i < nx / 2 ? i : i - nx;
        const double kx = kx1 * mx, ky = ky1 * j, k2 = kx * kx + ky * ky;
        const double ik2 = k2 > 0. ? 1. / k2 : 0.;
        const double wt = j == 0 ? 1. : 2.;
        const float2 c = w[q];
        const double ww = (double)c.x * c.x + (double)c.y * c.y;
        z += wt * ww;
        e += wt * ww * ik2;
        if (g) {
            const float2 f = g[q];
            p += wt * ik2 * ((double)c.x * f.x + (double)c.y * f.y);      // Re(psi^ conj g^)
        }
    }
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) {
        e += __shfl_xor(e, d, kWave);
        z += __shfl_xor(z, d, kWave);
        p += __shfl_xor(p, d, kWave);
    }
    const int wave = threadIdx.x / kWave;
    if (threadIdx.x % kWave == 0) { part[wave][0] = e; part[wave][1] = z; part[wave][2] = p; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double se = 0., sz = 0., sp = 0.;
        for (int k = 0; k < kDiagT / kWave; ++k) { se += part[k][0]; sz += part[k][1]; sp += part[k][2]; }
        double* o = out + 3 * (size_t)blockIdx.x;
        o[0] = 0.5 * se * inv_n2; o[1] = 0.5 * sz * inv_n2; o[2] = sp * inv_n2;
    }
}

// out[b] = (variance 1/2 <theta'^2>, dissipation kappa <|grad theta|^2>, flux_x <u theta'>, flux_y <v theta'>) over k != 0, u^ = i ky w^ / |k|^2,
// v^ = -i kx w^ / |k|^2: the same weights, normalisation, float64 sums and fixed order as ps_diag_kernel.
__global__ __launch_bounds__(kDiagT) void ps_scalar_diag_kernel(const float2* __restrict__ W, const float2* __restrict__ T, double* __restrict__ out,
                                                                 int nx, int my1, double kx1, double ky1, double kappa, double inv_n2) {
    __shared__ double part[kDiagT / kWave][4];
    const long per = (long)my1 * nx;
    const float2* w = W + (size_t)blockIdx.x * per;
    const float2* th = T + (size_t)blockIdx.x * per;
    double s[4] = {0., 0., 0., 0.};
    for (long q = threadIdx.x; q < per; q += kDiagT) {
        const int i = (int)(q % nx), j = (int)(q / nx);
        const int mx = i < nx / 2 ? i : i - nx;
        const double kx = kx1 * mx, ky = ky1 * j, k2 = kx * kx + ky * ky;
        const double ik2 = k2 > 0. ? 1. / k2 : 0.;
        const double wt = j == 0 ? 1. : 2.;
        const float2 c = w[q], d = th[q];
        const double tt = k2 > 0. ? (double)d.x * d.x + (double)d.y * d.y : 0.;
        const double cr = ((double)c.x * d.y - (double)c.y * d.x) * ik2;      // Re(i psi^ conj theta^)
        s[0] += wt * tt;
        s[1] += wt * tt * k2;
        s[2] += wt * ky * cr;
        s[3] -= wt * kx * cr;
    }
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] += __shfl_xor(s[k], d, kWave);
    }
    const int wave = threadIdx.x / kWave;
    if (threadIdx.x % kWave == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) part[wave][k] = s[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[4] = {0., 0., 0., 0.};
        for (int k = 0; k < kDiagT / kWave; ++k) { t[0] += part[k][0]; t[1] += part[k][1]; t[2] += part[k][2]; t[3] += part[k][3]; }
        double* o = out + 4 * (size_t)blockIdx.x;
        o[0] = 0.5 * t[0] * inv_n2; o[1] = kappa * t[1] * inv_n2; o[2] = t[2] * inv_n2; o[3] = t[3] * inv_n2;
    }
}

// out[b][k][l] (float64) = 1/2 sum wt Re(conj(d_k) d_l) / |k|^2 / (nx ny)^2 over the kept stored modes of grid b: the energy inner product of
// members k and l of D [K][B][my1][nx], whose diagonal is ps_diag_kernel's E of each member.  One workgroup per (grid, pair k <= l), which
// writes both triangles: symmetric by construction.  ps_diag_kernel's walk, float64 sums, shuffle tree and index-ordered partials: no
// atomics, so two runs give the same bits and a grid's numbers do not depend on its batch neighbours or on K.
__global__ __launch_bounds__(kDiagT) void ps_tangent_gram_kernel(const float2* __restrict__ D, double* __restrict__ out, int K, long kstride,
                                                                  int nx, int my1, double kx1, double ky1, double inv_n2) {
    __shared__ double part[kDiagT / kWave];
    int k = 0, rem = (int)blockIdx.x;                       // pair index -> (k, l), k <= l: row k holds K - k pairs
    while (rem >= K - k) { rem -= K - k; ++k; }
    const int l = k + rem;
    const long per = (long)my1 * nx;
    const float2* dk = D + (size_t)k * kstride + (size_t)blockIdx.y * per;
    const float2* dl = D + (size_t)l * kstride + (size_t)blockIdx.y * per;
    double e = 0.;
    for (long q = threadIdx.x; q < per; q += kDiagT) {
        const int i = (int)(q % nx), j = (int)(q / nx);
        const int mx = i < nx / 2 ? i : i - nx;
        const double kx = kx1 * mx, ky = ky1 * j, k2 = kx * kx + ky * ky;
        const double ik2 = k2 > 0. && 3 * (mx < 0 ? -mx : mx) < nx ? 1. / k2 : 0.;
        const double wt = j == 0 ? 1. : 2.;
        const float2 c = dk[q], d = dl[q];
        e += wt * ((double)c.x * d.x + (double)c.y * d.y) * ik2;
    }
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) e += __shfl_xor(e, d, kWave);
    const int wave = threadIdx.x / kWave;
    if (threadIdx.x % kWave == 0) part[wave] = e;
    __syncthreads();
    if (threadIdx.x == 0) {
        double se = 0.;
        for (int w = 0; w < kDiagT / kWave; ++w) se += part[w];
        double* o = out + (size_t)blockIdx.y * K * K;
        o[(size_t)k * K + l] = o[(size_t)l * K + k] = 0.5 * se * inv_n2;
    }
}

// d_k <- sum_{l <= k} C[b][l][k] d_l in place, C float64 [B][K][K] upper triangular.  Every stored entry (b, q) has one owning lane, which
// walks k from K - 1 down to 0: d_k needs only members l <= k, none of which that walk has overwritten yet.  The sum is float64, l ascending,
// rounded once; the members are read from memory each time (no array over K in registers), the coefficients are uniform loads.
__global__ __launch_bounds__(256) void ps_tangent_combine_kernel(float2* __restrict__ D, const double* __restrict__ C, int K, long kstride, long per) {
    const double* c = C + (size_t)blockIdx.y * K * K;
    float2* d = D + (size_t)blockIdx.y * per;
    for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < per; q += (long)gridDim.x * blockDim.x) {
        for (int k = K - 1; k >= 0; --k) {
            double sx = 0., sy = 0.;
            for (int l = 0; l <= k; ++l) {
                const float2 z = d[(size_t)l * kstride + q];
                const double f = c[(size_t)l * K + k];
                sx = fma(f, (double)z.x, sx);
                sy = fma(f, (double)z.y, sy);
            }
            d[(size_t)k * kstride + q] = make_float2((float)sx, (float)sy);
        }
    }
}

// ---------------------------------------------------------------------------------------------------- shell spectra and transfers
// Shells of width dk = min(kx1, ky1) centred on s dk: the mode (m_x, j) belongs to shell s = floor(|k| / dk + 1/2), in float64 (restatement:
// tests/pspec_spectrum_oracle.py).  nshell = shell of the band's corner + 1; shell 0 holds the (0, 0) mode alone, which contributes nothing.
struct PsShells {
    double kx1, ky1, dk, inv_n2;
    int nshell, nx, my1, kmx;     // kmx = (nx - 1) / 3: the kept |m_x|
};

__device__ __forceinline__ int ps_shell_of(const PsShells& g, int m, int j) {
    const double kx = g.kx1 * m, ky = g.ky1 * j;
    return (int)floor(sqrt(kx * kx + ky * ky) / g.dk + 0.5);
}

// The smallest |m_x| in [0, kmx + 1] of row j whose shell is >= sh: an estimate from the radius r = (sh - 1/2) dk, then fixed with the
// predicate that classifies a mode (ps_shell_of is monotone in |m_x|), so a mode is counted in exactly the shell the predicate names.
__device__ __forceinline__ int ps_first_in_shell(const PsShells& g, int j, int sh) {
    const double r = (sh - 0.5) * g.dk, ky = g.ky1 * j, t = r * r - ky * ky;
    int m = r > 0. && t > 0. ? (int)fmin(sqrt(t) / g.kx1, (double)(g.kmx + 1)) : 0;
    while (m > 0 && ps_shell_of(g, m - 1, j) >= sh) --m;
    while (m <= g.kmx && ps_shell_of(g, m, j) < sh) ++m;
    return m;
}

// out[b][Q][nshell] (float64) = per-shell sums of a per-mode value over the stored half spectrum [B][my1][nx], weight 1 on the j = 0 line and
// 2 on j > 0, normalised by (nx ny)^2.  ONE WAVE per (grid, shell): its lanes stride over the rows j that the annulus can reach; on a row
// the lane walks the |m_x| interval of the annulus (ps_first_in_shell) in ascending order, +m_x then -m_x, summing in float64; then a fixed
// wave64 shuffle tree.  Every kept mode is read exactly once, by the wave of its shell; no atomics and no partials shared between waves, so
// a grid's numbers repeat bitwise and depend neither on the batch, nor on the grid's place in it, nor on the launch geometry (which only
// decides which wave takes which (grid, shell)).  The last shell also takes whatever the predicate puts beyond it (nothing, unless the
// corner's shell differs by a rounding from the host's count), so the shells always sum to the totals of ps_diag_kernel.
//   TRANSFER = false: Q = 4, (E, Z, F, V) from w^ (a), theta^ (b, or NULL: V = 0) and g^ (c, or NULL: F = 0; cshared: one for the batch)
//   TRANSFER = true:  Q = 3, (T_E, T_Z, T_theta) from the real modal fields Re(conj w^ N^) (a) and Re(conj theta^ N_theta^) (b, or NULL)
template <bool TRANSFER>
__global__ __launch_bounds__(kT) void ps_shell_kernel(const void* __restrict__ a, const void* __restrict__ b, const void* __restrict__ c, int cshared,
                                                      double* __restrict__ out, PsShells g, long nunits) {
    constexpr int Q = TRANSFER ? 3 : 4;
    const int lane = threadIdx.x % kWave;
    const long per = (long)g.my1 * g.nx;
    for (long u = (long)blockIdx.x * kW + threadIdx.x / kWave; u < nunits; u += (long)gridDim.x * kW) {
        const long gb = u / g.nshell;
        const int s = (int)(u % g.nshell);
        const size_t base = (size_t)gb * per;
        // rows beyond (s + 1/2) dk / ky1 cannot reach the shell (one row of slack: the predicate decides)
        const double jtop = ((s + 0.5) * g.dk) / g.ky1 + 1.0;
        const int jend = s == g.nshell - 1 || jtop >= (double)g.my1 ? g.my1 : (int)jtop + 1;
        double acc[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) acc[q] = 0.;
        for (int j = lane; j < jend; j += kWave) {
            const int m0 = ps_first_in_shell(g, j, s);
            const int m1 = s == g.nshell - 1 ? g.kmx + 1 : ps_first_in_shell(g, j, s + 1);
            const double ky = g.ky1 * j, wt = j == 0 ? 1. : 2.;
            const size_t rowb = base + (size_t)j * g.nx;
            for (int m = m0; m < m1; ++m) {
                if ((m | j) == 0) continue;
                const double kx = g.kx1 * m, ik2 = 1. / (kx * kx + ky * ky);
                for (int sg = 0; sg < (m == 0 ? 1 : 2); ++sg) {
                    const size_t q = rowb + (sg == 0 ? m : g.nx - m);
                    if constexpr (TRANSFER) {
                        const double tw = static_cast<const float*>(a)[q];
                        acc[0] += wt * tw * ik2;
                        acc[1] += wt * tw;
                        if (b) acc[2] += wt * static_cast<const float*>(b)[q];
                    } else {
                        const float2 w = static_cast<const float2*>(a)[q];
                        const double ww = (double)w.x * w.x + (double)w.y * w.y;
                        acc[0] += wt * ww * ik2;
                        acc[1] += wt * ww;
                        if (c) {
                            const float2 f = static_cast<const float2*>(c)[cshared ? q - base : q];
                            acc[2] += wt * ik2 * ((double)w.x * f.x + (double)w.y * f.y);      // Re(psi^ conj g^)
                        }
                        if (b) {
                            const float2 d = static_cast<const float2*>(b)[q];
                            acc[3] += wt * ((double)d.x * d.x + (double)d.y * d.y);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int d = kWave / 2; d > 0; d >>= 1) {
#pragma unroll
            for (int q = 0; q < Q; ++q) acc[q] += __shfl_xor(acc[q], d, kWave);
        }
        if (lane == 0) {
            double* o = out + (size_t)gb * Q * g.nshell + s;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const double half = !TRANSFER && q != 2 ? 0.5 : 1.;          // E, Z and V carry the 1/2 of a quadratic mean
                o[(size_t)q * g.nshell] = half * acc[q] * g.inv_n2;
            }
        }
    }
}

// out[b][nshell] (float64) = the buoyancy production per shell, B(s) = sum wt Re(conj(bx u^ + by v^) theta^) / (nx ny)^2 with u^ = i ky psi^,
// v^ = -i kx psi^ from w^: Re(conj(i c psi^) theta^) = c Im(conj(psi^) theta^), c = bx ky - by kx.  ps_shell_kernel's sibling: its walk, its
// order of summation and its shuffle tree (one wave per (grid, shell), float64, no atomics), so the same determinism; summed over the shells it
// is bx flux_x + by flux_y of ps_scalar_diag_kernel.
__global__ __launch_bounds__(kT) void ps_buoyancy_shell_kernel(const float2* __restrict__ W, const float2* __restrict__ T, double* __restrict__ out,
                                                               PsShells g, long nunits, double bx, double by) {
    const int lane = threadIdx.x % kWave;
    const long per = (long)g.my1 * g.nx;
    for (long u = (long)blockIdx.x * kW + threadIdx.x / kWave; u < nunits; u += (long)gridDim.x * kW) {
        const long gb = u / g.nshell;
        const int s = (int)(u % g.nshell);
        const size_t base = (size_t)gb * per;
        const double jtop = ((s + 0.5) * g.dk) / g.ky1 + 1.0;
        const int jend = s == g.nshell - 1 || jtop >= (double)g.my1 ? g.my1 : (int)jtop + 1;
        double acc = 0.;
        for (int j = lane; j < jend; j += kWave) {
            const int m0 = ps_first_in_shell(g, j, s);
            const int m1 = s == g.nshell - 1 ? g.kmx + 1 : ps_first_in_shell(g, j, s + 1);
            const double ky = g.ky1 * j, wt = j == 0 ? 1. : 2.;
            const size_t rowb = base + (size_t)j * g.nx;
            for (int m = m0; m < m1; ++m) {
                if ((m | j) == 0) continue;
                const double kxa = g.kx1 * m, ik2 = 1. / (kxa * kxa + ky * ky);
                for (int sg = 0; sg < (m == 0 ? 1 : 2); ++sg) {
                    const size_t q = rowb + (sg == 0 ? m : g.nx - m);
                    const double kx = sg == 0 ? kxa : -kxa;
                    const float2 w = W[q], d = T[q];
                    acc += wt * (bx * ky - by * kx) * ik2 * ((double)w.x * d.y - (double)w.y * d.x);
                }
            }
        }
#pragma unroll
        for (int d = kWave / 2; d > 0; d >>= 1) acc += __shfl_xor(acc, d, kWave);
        if (lane == 0) out[(size_t)gb * g.nshell + s] = acc * g.inv_n2;
    }
}

// out[b][2][nshell] (float64) = the linear term's rates per shell, D_E(s) = sum wt Re(lambda_k) |w^_k|^2 / |k|^2 / (nx ny)^2 and D_Z(s) the same
// without 1 / |k|^2, so that dE/dt|linear = sum_s D_E and dZ/dt|linear = sum_s D_Z (E and Z carry a 1/2, d|w^|^2/dt = 2 Re(lambda) |w^|^2).
// rate = Re(lambda) float64 [my1][nx], shared by the batch.  ps_shell_kernel's sibling, as ps_buoyancy_shell_kernel is: its walk, its order
// of summation and its shuffle tree, so the same determinism.
__global__ __launch_bounds__(kT) void ps_linear_shell_kernel(const float2* __restrict__ W, const double* __restrict__ rate, double* __restrict__ out,
                                                             PsShells g, long nunits) {
    const int lane = threadIdx.x % kWave;
    const long per = (long)g.my1 * g.nx;
    for (long u = (long)blockIdx.x * kW + threadIdx.x / kWave; u < nunits; u += (long)gridDim.x * kW) {
        const long gb = u / g.nshell;
        const int s = (int)(u % g.nshell);
        const size_t base = (size_t)gb * per;
        const double jtop = ((s + 0.5) * g.dk) / g.ky1 + 1.0;
        const int jend = s == g.nshell - 1 || jtop >= (double)g.my1 ? g.my1 : (int)jtop + 1;
        double accE = 0., accZ = 0.;
        for (int j = lane; j < jend; j += kWave) {
            const int m0 = ps_first_in_shell(g, j, s);
            const int m1 = s == g.nshell - 1 ? g.kmx + 1 : ps_first_in_shell(g, j, s + 1);
            const double ky = g.ky1 * j, wt = j == 0 ? 1. : 2.;
            const size_t row = (size_t)j * g.nx;
            for (int m = m0; m < m1; ++m) {
                if ((m | j) == 0) continue;
                const double kx = g.kx1 * m, ik2 = 1. / (kx * kx + ky * ky);
                for (int sg = 0; sg < (m == 0 ? 1 : 2); ++sg) {
                    const size_t q = row + (sg == 0 ? m : g.nx - m);
                    const float2 w = W[base + q];
                    const double d = wt * rate[q] * ((double)w.x * w.x + (double)w.y * w.y);
                    accE += d * ik2;
                    accZ += d;
                }
            }
        }
#pragma unroll
        for (int d = kWave / 2; d > 0; d >>= 1) {
            accE += __shfl_xor(accE, d, kWave);
            accZ += __shfl_xor(accZ, d, kWave);
        }
        if (lane == 0) {
            double* o = out + (size_t)gb * 2 * g.nshell + s;
            o[0] = accE * g.inv_n2;
            o[g.nshell] = accZ * g.inv_n2;
        }
    }
}

// The column pass of a transfer evaluation: the tile and the staged forward transform of stages S >= 1 of ps_col_kernel (pspec_col_tile.inc
// without the pins of tx and tv, pspec_stage.inc); in place of the Lawson update it forms, per stored mode, Re(conj w^ N^) with N^ = -M P^
// (the step's mask: `keep` as in pspec_col_pass.inc) and, SCALAR, Re(conj theta^ N_theta^) from Ph's second field, and writes them as float32
// modal fields Tw, Tt [B][my1][nx].  It writes neither W nor Th.
template <int N, bool SCALAR>
__global__ __launch_bounds__(kT) void ps_transfer_kernel(const float2* __restrict__ Ph, const float2* __restrict__ W, const float2* __restrict__ Th,
                                                         float* __restrict__ Tw, float* __restrict__ Tt, PsArgs a) {
    using L = PsLds<N>;
    constexpr int TPF = L::TPF, CW = L::LINES, RPI = kT / CW;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const cf* tab = ps_tables<N>(smem);
    unsigned char* lines = smem + L::TAB_BYTES;
    const int my1 = a.my1;
    const long ntiles = (a.nlines + CW - 1) / CW;
    for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int tx = threadIdx.x;
#include "pspec_col_tile.inc"
        const int tv = tid;
        static_for<0, SCALAR ? 2 : 1>([&](auto fld) {
            constexpr bool TH = decltype(fld)::value == 1;
            const float2* ph = TH ? Ph + a.fstride : Ph;
            const float2* Ws = TH ? Th : W;
            float* To = TH ? Tt : Tw;
            cf z[16];
#include "pspec_stage.inc"
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                const int e = tv + TPF * m;
                const int mx = m < 8 ? e : e - N;
                const bool keep = lok && 3 * (mx < 0 ? -mx : mx) < N && (TH || (mx | lj) != 0);
                const float2 w = lok ? Ws[wbase + e] : make_float2(0.f, 0.f);
                const float v = keep ? -fmaf(w.x, z[m].x, w.y * z[m].y) : 0.f;              // Re(conj w^ N^), N^ = -P^
                if (lok) To[wbase + e] = v;
            }
            __syncthreads();                        // the next staging overwrites line images other waves may still read
        });
    }
}

// ---------------------------------------------------------------------------------------------------- host side
inline int kept_y(int ny) { return (ny - 1) / 3 + 1; }

inline unsigned grid_of(long work, long per) { return capped_grid((work + per - 1) / per, kGridCap); }

template <typename T, typename... X> constexpr bool has = (std::is_same_v<T, X> || ... || false);

// gr: nothing (the unscalared kernel), a PsGrad (the scalar one) or a PsBuoyGrad (the buoyant one)
template <int N, typename... Gr>
int launch_row(const float2* G, float2* Ph, const PsArgs& a, hipStream_t s, Gr... gr) {
    constexpr bool SC = sizeof...(Gr) == 1, BU = has<PsBuoyGrad, Gr...>;
    constexpr auto kern = ps_row_kernel<N, SC, BU, Gr...>;
    if (int rc = lds_opt_in<kern>(PsLds<N>::TOTAL, "spec_ns")) return rc;
    hipLaunchKernelGGL(kern, dim3(grid_of(a.nlines, PsLds<N>::LINES)), dim3(kT), PsLds<N>::TOTAL, s, G, Ph, a, gr...);
    return check_launch(BU ? "spec_ns buoyant row pass" : SC ? "spec_ns scalar row pass" : "spec_ns row pass");
}

template <int N>
int launch_row_tan(const float2* G, float2* Ph, const PsArgs& a, hipStream_t s) {
    constexpr auto kern = ps_row_tan_kernel<N>;
    if (int rc = lds_opt_in<kern>(PsLds<N>::TOTAL, "spec_ns")) return rc;
    hipLaunchKernelGGL(kern, dim3(grid_of(a.nlines, PsLds<N>::LINES)), dim3(kT), PsLds<N>::TOTAL, s, G, Ph, a);
    return check_launch("spec_ns tangent row pass");
}

// gr: a PsGrad (the passive scalar's tangent) or a PsBuoyGrad (the buoyant one's)
template <int N, typename Gr>
int launch_row_tan_scalar(const float2* G, float2* Ph, const PsArgs& a, hipStream_t s, Gr gr) {
    constexpr bool BU = std::is_same_v<Gr, PsBuoyGrad>;
    constexpr auto kern = ps_row_tan_scalar_kernel<N, BU>;
    if (int rc = lds_opt_in<kern>(PsLds<N>::TOTAL, "spec_ns")) return rc;
    hipLaunchKernelGGL(kern, dim3(grid_of(a.nlines, PsLds<N>::LINES)), dim3(kT), PsLds<N>::TOTAL, s, G, Ph, a, gr);
    return check_launch(BU ? "spec_ns buoyant tangent row pass" : "spec_ns scalar tangent row pass");
}

template <int N>
int launch_row_tans(const float2* G, float2* Ph, const PsArgs& a, int K, hipStream_t s) {
    constexpr auto kern = ps_row_tans_kernel<N>;
    if (int rc = lds_opt_in<kern>(PsLds<N>::TOTAL, "spec_ns")) return rc;
    hipLaunchKernelGGL(kern, dim3(grid_of(a.nlines, PsLds<N>::LINES)), dim3(kT), PsLds<N>::TOTAL, s, G, Ph, a, K);
    return check_launch("spec_ns tangents row pass");
}

template <int N, typename Gr>
int launch_row_tans_scalar(const float2* G, float2* Ph, const PsArgs& a, int K, hipStream_t s, Gr gr) {
    constexpr bool BU = std::is_same_v<Gr, PsBuoyGrad>;
    constexpr auto kern = ps_row_tans_scalar_kernel<N, BU>;
    if (int rc = lds_opt_in<kern>(PsLds<N>::TOTAL, "spec_ns")) return rc;
    hipLaunchKernelGGL(kern, dim3(grid_of(a.nlines, PsLds<N>::LINES)), dim3(kT), PsLds<N>::TOTAL, s, G, Ph, a, gr, K);
    return check_launch(BU ? "spec_ns buoyant tangents row pass" : "spec_ns scalar tangents row pass");
}

// The column kernel of stage S whose argument pack ends in x...: a PsScalar (the SCALAR kernels), a PsTangent or a PsTangents, a PsLinear, a PsStoch, in that order, each or
// none; a PsTangentScalar follows a PsScalar and a PsTangent, a PsTangentsScalar a PsScalar and a PsTangents.  fc is read only by the FORCED kernels.
template <int N, int S, bool FORCED, typename... X>
int launch_col(const float2* Ph, float2* G, float2* W, float2* A, const float* mean, const PsArgs& a, int emit, const PsForce* fc,
               hipStream_t s, X... x) {
    constexpr bool SC = has<PsScalar, X...>, LI = has<PsLinear, X...>, ST = has<PsStoch, X...>, KE = has<PsKeep, X...> || has<PsKeepScalar, X...> || has<PsKeepTangent, X...>;
    constexpr bool TA = has<PsTangent, X...>, TS = has<PsTangents, X...>, TT = has<PsTangentScalar, X...>, TU = has<PsTangentsScalar, X...>;
    constexpr auto kern = ps_col_kernel<N, S, FORCED, SC, X...>;
    std::conditional_t<FORCED, PsForce, PsNoForce> f{};
    if constexpr (FORCED) f = *fc;
    if (int rc = lds_opt_in<kern>(PsLds<N>::TOTAL, "spec_ns")) return rc;
    hipLaunchKernelGGL(kern, dim3(grid_of(a.nlines, PsLds<N>::LINES)), dim3(kT), PsLds<N>::TOTAL, s, Ph, G, W, A, mean, a, emit, f, x...);
    return check_launch(TU       ? "spec_ns scalar tangents column pass"
                        : TS     ? "spec_ns tangents column pass"
                        : TT     ? "spec_ns scalar tangent column pass"
                        : TA     ? (KE ? "spec_ns stage-keeping tangent column pass" : "spec_ns tangent column pass")
                        : KE     ? "spec_ns stage-keeping column pass"
                        : LI     ? (SC ? "spec_ns linear scalar column pass" : "spec_ns linear column pass")
                        : ST     ? (SC ? "spec_ns stochastic scalar column pass" : "spec_ns stochastic column pass")
                        : SC     ? "spec_ns scalar column pass"
                        : FORCED ? "spec_ns forced column pass"
                                 : "spec_ns column pass");
}

// f(std::integral_constant<int, S>) of a run-time stage S in [LO, HI]; a stage beyond takes HI
template <int LO, int HI, typename F>
int with_stage(int S, F&& f) {
    if constexpr (LO == HI) return f(std::integral_constant<int, HI>{});
    else return S == LO ? f(std::integral_constant<int, LO>{}) : with_stage<LO + 1, HI>(S, f);
}

// The one place where a stage's run-time facts become a kernel.  fc == nullptr: the unforced kernels (stage 0 has no other form); sc: the
// SCALAR ones; li (with fc): a linear step, whose stages 1-3 are the LINEAR kernels (stage 4 applies no factor); st (with fc): a stochastic
// step, whose stages 1 and 4 are the STOCH kernels; tg (with sc only beside tt): the TANGENT ones, of every stage and form; tt (with sc
// and tg): those of the scalar system's tangent, which live in pspec_scalar_tangent.hip and are reached through ps_scalar_tangent_col; ts (never with tg; with sc only beside tu): the TANGENTS ones, likewise;
// tu (with sc and ts): those of K tangents on the scalar system, which live in pspec_scalar_tangents.hip and are reached through ps_scalar_tangents_col.  The pack grows in the kernel's order, and a form no step has is never named.
template <int N>
int launch_col_stage(int S, const float2* Ph, float2* G, float2* W, float2* A, const float* mean, const PsArgs& a, int emit, const PsForce* fc,
                     const PsScalar* sc, hipStream_t s, const PsStoch* st = nullptr, const PsLinear* li = nullptr, const PsTangent* tg = nullptr,
                     const PsTangents* ts = nullptr, const PsTangentScalar* tt = nullptr, const PsTangentsScalar* tu = nullptr) {
#ifndef PSPEC_KERNEL_TU
    if (tt) return ps_scalar_tangent_col(N, S, Ph, G, W, A, mean, &a, emit, fc, sc, s, st, li, tg, tt);
    if (tu) return ps_scalar_tangents_col(N, S, Ph, G, W, A, mean, &a, emit, fc, sc, s, st, li, ts, tu);
#endif
    auto stage = [&](auto stage_c) {
        constexpr int K = decltype(stage_c)::value;
        auto stoch = [&](auto forced, auto... x) {
            constexpr bool F = decltype(forced)::value;
            if constexpr (F && (K == 1 || K == 4))
                if (st) return launch_col<N, K, F>(Ph, G, W, A, mean, a, emit, fc, s, x..., *st);
            return launch_col<N, K, F>(Ph, G, W, A, mean, a, emit, fc, s, x...);
        };
        auto linear = [&](auto forced, auto... x) {
            if constexpr (decltype(forced)::value && K >= 1 && K <= 3)
                if (li) return stoch(forced, x..., *li);
            return stoch(forced, x...);
        };
#if defined(PSPEC_SCALAR_TANGENT_TU)      // this translation unit names the forms with a PsTangentScalar and no other
        auto scalar = [&](auto forced) { return linear(forced, *sc, *tg, *tt); };
#elif defined(PSPEC_SCALAR_TANGENTS_TU)   // and this one those with a PsTangentsScalar
        auto scalar = [&](auto forced) { return linear(forced, *sc, *ts, *tu); };
#else
        auto scalar = [&](auto forced) { return ts ? linear(forced, *ts) : tg ? linear(forced, *tg) : sc ? linear(forced, *sc) : linear(forced); };
#endif
        if constexpr (K >= 1)
            if (fc) return scalar(std::true_type{});
        return scalar(std::false_type{});
    };
    return with_stage<0, 4>(S, stage);
}

// Stage S = 1..3 of the adjoint's recomputation: the plain, the forced or (li, with fc) the linear kernel with the stage store (launch_col_stage
// never names this form).  keep: a PsKeep, or with a scalar a PsKeepScalar and sc the PsScalar; the pack grows in the kernel's order.
template <int N, typename Keep, typename... Sc>
int launch_col_keep(int S, const float2* Ph, float2* G, float2* W, float2* A, const float* mean, const PsArgs& a, const PsForce* fc,
                    const PsLinear* li, hipStream_t s, Keep keep, Sc... sc) {
    auto go = [&](auto stage_c) {
        constexpr int K = decltype(stage_c)::value;
        if (fc && li) return launch_col<N, K, true>(Ph, G, W, A, mean, a, 1, fc, s, sc..., *li, keep);
        return fc ? launch_col<N, K, true>(Ph, G, W, A, mean, a, 1, fc, s, sc..., keep) : launch_col<N, K, false>(Ph, G, W, A, mean, a, 1, fc, s, sc..., keep);
    };
    return with_stage<1, 3>(S, go);
}

template <int N>
int launch_row_adj2(const float2* G, float2* Ph, const PsArgs& a, hipStream_t s) {
    constexpr auto kern = ps_row_adj2_kernel<N>;
    if (int rc = lds_opt_in<kern>(PsLds<N>::TOTAL, "spec_ns")) return rc;
    hipLaunchKernelGGL(kern, dim3(grid_of(a.nlines, PsLds<N>::LINES)), dim3(kT), PsLds<N>::TOTAL, s, G, Ph, a);
    return check_launch("spec_ns second-order adjoint row pass");
}

// gr: nothing, or with a scalar a PsAdjGrad
template <int N, typename... Gr>
int launch_row_adj(const float2* G, float2* Ph, const PsArgs& a, hipStream_t s, Gr... gr) {
    constexpr bool SC = sizeof...(Gr) == 1;
    constexpr auto kern = ps_row_adj_kernel<N, SC, Gr...>;
    if (int rc = lds_opt_in<kern>(PsLds<N>::TOTAL, "spec_ns")) return rc;
    hipLaunchKernelGGL(kern, dim3(grid_of(a.nlines, PsLds<N>::LINES)), dim3(kT), PsLds<N>::TOTAL, s, G, Ph, a, gr...);
    return check_launch(SC ? "spec_ns scalar adjoint row pass" : "spec_ns adjoint row pass");
}

// ad: a PsAdj, or with a scalar a PsAdjScalar; a PsAdjLinear / PsAdjScalarLinear for stages 3-1 of a linear step's adjoint (no other stage has that form),
// or there a PsAdjOperator / PsAdjScalarOperator when the table's cotangent is wanted; a PsAdjSecond, or for stages 3-1 of a linear step a
// PsAdjSecondLinear: the second-order adjoint's (named in pspec_second_adjoint.hip only)
template <int N, typename Ad>
int launch_col_adj(int S, const float2* Ph, float2* G, const float* mean, const PsArgs& a, const Ad& ad, hipStream_t s) {
    constexpr bool SC = std::is_base_of_v<PsAdjScalar, Ad>, SE = std::is_base_of_v<PsAdjSecond, Ad>;
    constexpr bool LI = std::is_base_of_v<PsAdjLinear, Ad> || std::is_base_of_v<PsAdjScalarLinear, Ad> || std::is_base_of_v<PsAdjSecondLinear, Ad>;
    auto go = [&](auto stage_c) {
        constexpr auto kern = ps_col_adj_kernel<N, decltype(stage_c)::value, Ad>;
        if (int rc = lds_opt_in<kern>(PsLds<N>::TOTAL, "spec_ns")) return rc;
        hipLaunchKernelGGL(kern, dim3(grid_of(a.nlines, PsLds<N>::LINES)), dim3(kT), PsLds<N>::TOTAL, s, Ph, G, mean, a, ad);
        return check_launch(SE   ? (LI ? "spec_ns linear second-order adjoint column pass" : "spec_ns second-order adjoint column pass")
                            : LI ? (SC ? "spec_ns linear scalar adjoint column pass" : "spec_ns linear adjoint column pass")
                            : SC ? "spec_ns scalar adjoint column pass"
                                 : "spec_ns adjoint column pass");
    };
    return with_stage<LI ? 1 : 0, LI ? 3 : 4>(S, go);
}

size_t step_bytes(int batch, int nx, int ny) { return (size_t)6 * batch * nx * kept_y(ny) * sizeof(float2); }
size_t init_bytes(int batch, int nx, int ny) { return (size_t)2 * batch * nx * (ny / 2 + 1) * sizeof(float2); }
size_t fields_bytes(int batch, int nx, int ny) {
    return (size_t)6 * batch * nx * (ny / 2 + 1) * sizeof(float2) + (size_t)4 * batch * nx * ny * sizeof(float);
}
size_t work_bytes(int batch, int nx, int ny) {
    size_t b = step_bytes(batch, nx, ny);
    if (init_bytes(batch, nx, ny) > b) b = init_bytes(batch, nx, ny);
    if (fields_bytes(batch, nx, ny) > b) b = fields_bytes(batch, nx, ny);
    return b;
}

// the scalar step's A, A_theta, G[6], Ph[2]: 10 compacted fields against 6 (its init and field need one rfft2 spectrum: inside work_bytes)
size_t scalar_work_bytes(int batch, int nx, int ny) {
    const size_t b = work_bytes(batch, nx, ny), st = (size_t)10 * batch * nx * kept_y(ny) * sizeof(float2);
    return st > b ? st : b;
}

// A layout of work in compacted fields of fstride complex each, in this order: the accumulators, G, Ph, the adjoint's kept stage states.
//   the step:            A, G[4], Ph;   with a scalar A, A_theta, G[6], Ph[2]
//   the flow's adjoint:  A, wbar in A_theta's place, G[6], Ph[2] (the recomputation's launches use the first 4 and 1 of them), s1, s2, s3: 13
//   the scalar adjoint:  A, A_theta (wbar and thetabar once the stages are recomputed), G[10], Ph[3] (the recomputation's: 6 and 2), s1, s2, s3
//                        of w^, then of theta^: 21
//   the tangent step:    A, dA in A_theta's place, G[8], Ph[2]: 12
//   the scalar tangent:  A, A_theta, dA, dA_theta, G[12], Ph[4]: 20
//   the second adjoint:  A, dA (wbar and dwbar once the stages are recomputed), G[12], Ph[4] (the recomputation's, the tangent step's: 8 and 2),
//                        s1, s2, s3 of w^, then d1, d2, d3 of dw^: 24
//   K tangents:          A, dA[K], G[4 + 4K], Ph[1 + K]: 6 + 6K (tangents_layout; K = 1 is the tangent step's)
//   K tangents, scalar:  A, A_theta, dA[K], dA_theta[K], G[6 + 6K], Ph[2 + 2K]: 10 + 10K (scalar_tangents_layout; K = 1 is the scalar tangent's)
struct PsLayout {
    int acc, g, ph, keep;
    constexpr int fields() const { return acc + g + ph + keep; }
};
constexpr PsLayout kLayFlow{1, 4, 1, 0}, kLayScalar{2, 6, 2, 0}, kLayAdjoint{2, 6, 2, 3}, kLayScalarAdjoint{2, 10, 3, 6}, kLayTangent{2, 8, 2, 0},
                   kLayScalarTangent{4, 12, 4, 0}, kLaySecondAdjoint{2, 12, 4, 6};

size_t layout_work_bytes(const PsLayout& lay, int batch, int nx, int ny) {
    const size_t b = work_bytes(batch, nx, ny), st = (size_t)lay.fields() * batch * nx * kept_y(ny) * sizeof(float2);
    return st > b ? st : b;
}
size_t adjoint_work_bytes(int batch, int nx, int ny) { return layout_work_bytes(kLayAdjoint, batch, nx, ny); }
size_t scalar_adjoint_work_bytes(int batch, int nx, int ny) { return layout_work_bytes(kLayScalarAdjoint, batch, nx, ny); }
size_t tangent_work_bytes(int batch, int nx, int ny) { return layout_work_bytes(kLayTangent, batch, nx, ny); }
size_t scalar_tangent_work_bytes(int batch, int nx, int ny) { return layout_work_bytes(kLayScalarTangent, batch, nx, ny); }
size_t second_adjoint_work_bytes(int batch, int nx, int ny) { return layout_work_bytes(kLaySecondAdjoint, batch, nx, ny); }
constexpr int kMaxTangents = 32;
constexpr PsLayout tangents_layout(int K) { return PsLayout{1 + K, 4 + 4 * K, 1 + K, 0}; }
size_t tangents_work_bytes(int batch, int ntan, int nx, int ny) { return layout_work_bytes(tangents_layout(ntan), batch, nx, ny); }
constexpr PsLayout scalar_tangents_layout(int K) { return PsLayout{2 + 2 * K, 6 + 6 * K, 2 + 2 * K, 0}; }
size_t scalar_tangents_work_bytes(int batch, int ntan, int nx, int ny) { return layout_work_bytes(scalar_tangents_layout(ntan), batch, nx, ny); }

// The fields of a layout in work, and the arguments of the column pass (col) and of the row pass (row).
struct PsWork {
    float2 *A, *At, *G, *Ph, *keep;
    PsArgs col, row;
    PsWork(void* work, int batch, int nx, int ny, const PsLayout& lay, double Lx, double Ly, float hnudt, float dt) {
        const int my1 = kept_y(ny);
        const long fstride = (long)batch * nx * my1;
        A = static_cast<float2*>(work);
        At = A + fstride;
        G = A + lay.acc * fstride;
        Ph = G + lay.g * fstride;
        keep = Ph + lay.ph * fstride;
        col = PsArgs{(long)batch * my1, fstride, my1, (float)(2.0 * M_PI / Lx), (float)(2.0 * M_PI / Ly), hnudt, dt, (float)(1.0 / ((double)nx * ny))};
        row = col;
        row.nlines = (long)batch * nx;
    }
    PsWork(void* work, int batch, int nx, int ny, bool scalar, double Lx, double Ly, float hnudt, float dt)
        : PsWork(work, batch, nx, ny, scalar ? kLayScalar : kLayFlow, Lx, Ly, hnudt, dt) {}
};

int check_lengths(const char* what, double Lx, double Ly) {
    if (!(Lx > 0) || !(Ly > 0) || !std::isfinite(Lx) || !std::isfinite(Ly))
        return fail(NNS_ERR_INVALID_ARG, "%s: Lx = %g, Ly = %g must be positive and finite", what, Lx, Ly);
    return NNS_OK;
}

int check_axes(const char* what, int nx, int ny) {
    if (!pow2_in_range(nx) || !pow2_in_range(ny))
        return fail(NNS_ERR_UNSUPPORTED, "%s: nx = %d, ny = %d: each axis must be a power of two in [64, 1024]", what, nx, ny);
    return NNS_OK;
}

// box and axes: what every call checks before it looks at a workspace or a shell count
int check_box(const char* what, int nx, int ny, double Lx, double Ly) {
    if (int rc = check_lengths(what, Lx, Ly)) return rc;
    return check_axes(what, nx, ny);
}

enum PsWorkKind { kWorkFlow = 0, kWorkScalar = 1, kWorkAdjoint = 2, kWorkScalarAdjoint = 3, kWorkTangent = 4, kWorkTangents = 5, kWorkScalarTangent = 6, kWorkScalarTangents = 7, kWorkSecondAdjoint = 8 };      // a bool converts: false the flow's workspace, true the scalar's

int check_work(const char* what, int batch, int nx, int ny, size_t wbytes, int kind, int ntan = 0) {      // ntan: kWorkTangents' and kWorkScalarTangents' K
    const size_t need = kind == kWorkSecondAdjoint ? second_adjoint_work_bytes(batch, nx, ny)
                        : kind == kWorkScalarTangents ? scalar_tangents_work_bytes(batch, ntan, nx, ny)
                        : kind == kWorkScalarTangent ? scalar_tangent_work_bytes(batch, nx, ny)
                        : kind == kWorkTangents    ? tangents_work_bytes(batch, ntan, nx, ny)
                        : kind == kWorkTangent     ? tangent_work_bytes(batch, nx, ny)
                        : kind == kWorkScalarAdjoint ? scalar_adjoint_work_bytes(batch, nx, ny)
                        : kind == kWorkAdjoint     ? adjoint_work_bytes(batch, nx, ny)
                        : kind == kWorkScalar      ? scalar_work_bytes(batch, nx, ny)
                                                   : work_bytes(batch, nx, ny);
    if (wbytes < need)
        return fail(NNS_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed (%s)", what, wbytes, need,
                    kind == kWorkSecondAdjoint ? "nns_spec_ns_second_adjoint_workspace"
                    : kind == kWorkScalarTangents ? "nns_spec_ns_scalar_tangents_workspace"
                    : kind == kWorkScalarTangent ? "nns_spec_ns_scalar_tangent_workspace"
                    : kind == kWorkTangents    ? "nns_spec_ns_tangents_workspace"
                    : kind == kWorkTangent     ? "nns_spec_ns_tangent_workspace"
                    : kind == kWorkScalarAdjoint ? "nns_spec_ns_scalar_adjoint_workspace"
                    : kind == kWorkAdjoint     ? "nns_spec_ns_adjoint_workspace"
                    : kind == kWorkScalar      ? "nns_spec_ns_scalar_workspace"
                                               : "nns_spec_ns_workspace");
    return NNS_OK;
}

int check_common(const char* what, int batch, int nx, int ny, double Lx, double Ly, size_t wbytes, int kind = kWorkFlow, int ntan = 0) {
    if (int rc = check_box(what, nx, ny, Lx, Ly)) return rc;
    return check_work(what, batch, nx, ny, wbytes, kind, ntan);
}

// dt, nu, drag and nsteps of a step, forward or adjoint
int check_step_numbers(const char* who, double dt, double nu, double drag, int nsteps) {
    if (!(dt > 0) || !std::isfinite(dt) || !(nu >= 0) || !std::isfinite(nu) || nsteps < 0)
        return fail(NNS_ERR_INVALID_ARG, "%s: dt = %g must be > 0, nu = %g >= 0, nsteps = %d >= 0", who, dt, nu, nsteps);
    if (!(drag >= 0) || !std::isfinite(drag)) return fail(NNS_ERR_INVALID_ARG, "%s: drag = %g must be finite and >= 0", who, drag);
    return NNS_OK;
}

int check_gbatch(const char* what, const float* ghat, int gbatch, int batch) {
    if (ghat ? (gbatch != 1 && gbatch != batch) : gbatch != 0)
        return fail(NNS_ERR_INVALID_ARG, "%s: gbatch = %d must be 0 without ghat, 1 or batch = %d with it", what, gbatch, batch);
    return NNS_OK;
}

int check_buoyancy(const char* what, double bx, double by) {
    if (!std::isfinite(bx) || !std::isfinite(by)) return fail(NNS_ERR_INVALID_ARG, "%s: the buoyancy (%g, %g) must be finite", what, bx, by);
    return NNS_OK;
}

// kappa and G of a step with a scalar, forward or adjoint
int check_scalar_numbers(const char* who, double kappa, double gx, double gy) {
    if (!(kappa >= 0) || !std::isfinite(kappa) || !std::isfinite(gx) || !std::isfinite(gy))
        return fail(NNS_ERR_INVALID_ARG, "%s: kappa = %g must be finite and >= 0, the gradient (%g, %g) finite", who, kappa, gx, gy);
    return NNS_OK;
}

inline unsigned pw_grid(long n) { return capped_grid((n + 255) / 256, 4096); }

// dk and the shell count of a box: the shell of the band's corner (|m_x| = (nx - 1) / 3, j = my1 - 1) + 1, by the device's predicate
PsShells shells_of(int nx, int ny, double Lx, double Ly) {
    PsShells g{};
    g.kx1 = 2.0 * M_PI / Lx;
    g.ky1 = 2.0 * M_PI / Ly;
    g.dk = g.kx1 < g.ky1 ? g.kx1 : g.ky1;
    const double n = (double)nx * ny;
    g.inv_n2 = 1.0 / (n * n);
    g.nx = nx;
    g.my1 = kept_y(ny);
    g.kmx = (nx - 1) / 3;
    const double kx = g.kx1 * g.kmx, ky = g.ky1 * (g.my1 - 1);
    g.nshell = (int)std::floor(std::sqrt(kx * kx + ky * ky) / g.dk + 0.5) + 1;
    return g;
}

// box, axes, then the shell count: what the spectrum and transfer calls check before they look at a workspace
int check_shells(const char* what, int nx, int ny, double Lx, double Ly, int nshell, PsShells* g) {
    if (int rc = check_box(what, nx, ny, Lx, Ly)) return rc;
    *g = shells_of(nx, ny, Lx, Ly);
    if (nshell != g->nshell)
        return fail(NNS_ERR_INVALID_ARG, "%s: nshell = %d, this box has %d shells (nns_spec_ns_shells)", what, nshell, g->nshell);
    return NNS_OK;
}

// one wave per (grid, shell): the grid only decides which wave takes which
inline dim3 shell_grid(long nunits) { return dim3(capped_grid((nunits + kW - 1) / kW, 8 * kGridCap)); }

template <bool TRANSFER>
int launch_shells(const void* a, const void* b, const void* c, int cshared, double* out, const PsShells& g, int batch, hipStream_t s) {
    const long nunits = (long)batch * g.nshell;
    hipLaunchKernelGGL(ps_shell_kernel<TRANSFER>, shell_grid(nunits), dim3(kT), 0, s, a, b, c, cshared, out, g, nunits);
    return check_launch(TRANSFER ? "spec_ns_transfer shells" : "spec_ns_spectrum");
}

template <int N>
int launch_transfer(const float2* Ph, const float2* W, const float2* Th, float* Tw, float* Tt, const PsArgs& a, hipStream_t s) {
    const dim3 grid(grid_of(a.nlines, PsLds<N>::LINES));
    if (Th) {
        constexpr auto kern = ps_transfer_kernel<N, true>;
        if (int rc = lds_opt_in<kern>(PsLds<N>::TOTAL, "spec_ns")) return rc;
        hipLaunchKernelGGL(kern, grid, dim3(kT), PsLds<N>::TOTAL, s, Ph, W, Th, Tw, Tt, a);
        return check_launch("spec_ns_transfer scalar column pass");
    }
    constexpr auto kern = ps_transfer_kernel<N, false>;
    if (int rc = lds_opt_in<kern>(PsLds<N>::TOTAL, "spec_ns")) return rc;
    hipLaunchKernelGGL(kern, grid, dim3(kT), PsLds<N>::TOTAL, s, Ph, W, Th, Tw, Tt, a);
    return check_launch("spec_ns_transfer column pass");
}

}  // namespace

#ifndef PSPEC_KERNEL_TU
NNS_API int nns_spec_ns_shells(int nx, int ny, double Lx, double Ly, int* nshell, double* dk) {
    if (!nshell || !dk) return fail(NNS_ERR_INVALID_ARG, "spec_ns_shells: nshell and dk must be non-NULL");
    if (int rc = check_box("spec_ns_shells", nx, ny, Lx, Ly)) return rc;
    const PsShells g = shells_of(nx, ny, Lx, Ly);
    *nshell = g.nshell;
    *dk = g.dk;
    return NNS_OK;
}

NNS_API int nns_spec_ns_spectrum_f32(const float* what, const float* that, const float* ghat, int gbatch, double* out, int nshell, int batch,
                                     int nx, int ny, double Lx, double Ly, void* stream) {
    if (!what || !out || batch < 1) return fail(NNS_ERR_INVALID_ARG, "spec_ns_spectrum: NULL pointer or batch < 1");
    if (int rc = check_gbatch("spec_ns_spectrum", ghat, gbatch, batch)) return rc;
    PsShells g;
    if (int rc = check_shells("spec_ns_spectrum", nx, ny, Lx, Ly, nshell, &g)) return rc;
    return launch_shells<false>(what, that, ghat, gbatch == 1 && batch > 1 ? 1 : 0, out, g, batch, as_stream(stream));
}

NNS_API int nns_spec_ns_buoyancy_spectrum_f32(const float* what, const float* that, double* out, int nshell, int batch, int nx, int ny, double Lx,
                                              double Ly, double bx, double by, void* stream) {
    if (!what || !that || !out || batch < 1) return fail(NNS_ERR_INVALID_ARG, "spec_ns_buoyancy_spectrum: NULL pointer or batch < 1");
    if (int rc = check_buoyancy("spec_ns_buoyancy_spectrum", bx, by)) return rc;
    PsShells g;
    if (int rc = check_shells("spec_ns_buoyancy_spectrum", nx, ny, Lx, Ly, nshell, &g)) return rc;
    const long nunits = (long)batch * g.nshell;
    hipLaunchKernelGGL(ps_buoyancy_shell_kernel, shell_grid(nunits), dim3(kT), 0, as_stream(stream), reinterpret_cast<const float2*>(what), reinterpret_cast<const float2*>(that), out, g, nunits, bx, by);
    return check_launch("spec_ns_buoyancy_spectrum");
}

NNS_API int nns_spec_ns_linear_spectrum_f32(const float* what, const double* rate, double* out, int nshell, int batch, int nx, int ny, double Lx,
                                            double Ly, void* stream) {
    if (!what || !rate || !out || batch < 1) return fail(NNS_ERR_INVALID_ARG, "spec_ns_linear_spectrum: NULL pointer or batch < 1");
    PsShells g;
    if (int rc = check_shells("spec_ns_linear_spectrum", nx, ny, Lx, Ly, nshell, &g)) return rc;
    const long nunits = (long)batch * g.nshell;
    hipLaunchKernelGGL(ps_linear_shell_kernel, shell_grid(nunits), dim3(kT), 0, as_stream(stream), reinterpret_cast<const float2*>(what), rate, out, g, nunits);
    return check_launch("spec_ns_linear_spectrum");
}

NNS_API int nns_spec_ns_transfer_f32(const float* what, const float* that, double* out, int nshell, void* work, size_t work_bytes_, int batch,
                                     int nx, int ny, double Lx, double Ly, void* stream) {
    if (!what || !out || !work || batch < 1) return fail(NNS_ERR_INVALID_ARG, "spec_ns_transfer: NULL pointer or batch < 1");
    PsShells g;
    if (int rc = check_shells("spec_ns_transfer", nx, ny, Lx, Ly, nshell, &g)) return rc;
    if (int rc = check_work("spec_ns_transfer", batch, nx, ny, work_bytes_, that != nullptr)) return rc;
    hipStream_t s = as_stream(stream);
    // the step's layout of work.  The accumulators are free here: the modal fields Re(conj w^ N^), Re(conj theta^ N_theta^) take the first
    // half of A's and A_theta's slots (float32 against complex), the zero mean of the co-moving frame a corner of A's second half
    const PsWork L(work, batch, nx, ny, that != nullptr, Lx, Ly, 0.f, 0.f);
    float* Tw = reinterpret_cast<float*>(L.A);
    float* Tt = that ? reinterpret_cast<float*>(L.At) : nullptr;
    float* zero_mean = Tw + L.col.fstride;
    void* zb[1] = {zero_mean};
    const long zn[1] = {(long)(2 * batch * sizeof(float))};
    if (int rc = zero_buffers(zb, zn, 1, s)) return rc;
    float2* W = const_cast<float2*>(reinterpret_cast<const float2*>(what));       // stage 0 only reads W / Th (its signature is the step's)
    const float2* Th = reinterpret_cast<const float2*>(that);
    const PsScalar scalar{const_cast<float2*>(Th), nullptr, 0.f};
    const PsGrad grad{0.f, 0.f};                                                  // the scalar's row pass without a gradient: advection alone
    if (int rc = dispatch_pow2(nx, "spec_ns", [&](auto n) {
            return launch_col_stage<decltype(n)::value>(0, L.Ph, L.G, W, nullptr, zero_mean, L.col, 1, nullptr, that ? &scalar : nullptr, s);
        }))
        return rc;
    if (int rc = dispatch_pow2(ny, "spec_ns", [&](auto n) {
            return that ? launch_row<decltype(n)::value>(L.G, L.Ph, L.row, s, grad) : launch_row<decltype(n)::value>(L.G, L.Ph, L.row, s);
        }))
        return rc;
    if (int rc = dispatch_pow2(nx, "spec_ns", [&](auto n) { return launch_transfer<decltype(n)::value>(L.Ph, W, Th, Tw, Tt, L.col, s); })) return rc;
    return launch_shells<true>(Tw, Tt, nullptr, 0, out, g, batch, s);
}

NNS_API int nns_spec_ns_workspace(int batch, int nx, int ny, size_t* bytes) {
    if (!bytes || batch < 1) return fail(NNS_ERR_INVALID_ARG, "spec_ns_workspace: bytes must be non-NULL and batch >= 1 (batch = %d)", batch);
    if (int rc = check_axes("spec_ns_workspace", nx, ny)) return rc;
    *bytes = work_bytes(batch, nx, ny);
    return NNS_OK;
}

NNS_API int nns_spec_ns_init_f32(const float* u, const float* v, float* what, float* mean, void* work, size_t work_bytes_, int batch,
                                 int nx, int ny, double Lx, double Ly, void* stream) {
    if (!u || !v || !what || !mean || !work || batch < 1) return fail(NNS_ERR_INVALID_ARG, "spec_ns_init: NULL pointer or batch < 1");
    if (int rc = check_common("spec_ns_init", batch, nx, ny, Lx, Ly, work_bytes_)) return rc;
    hipStream_t s = as_stream(stream);
    float* uh = static_cast<float*>(work);
    float* vh = uh + (size_t)2 * batch * nx * (ny / 2 + 1);
    if (int rc = nns_spec_rfft2_f32(u, uh, batch, nx, ny, stream)) return rc;
    if (int rc = nns_spec_rfft2_f32(v, vh, batch, nx, ny, stream)) return rc;
    const int my1 = kept_y(ny);
    hipLaunchKernelGGL(ps_init_kernel, dim3(pw_grid((long)batch * my1 * nx)), dim3(256), 0, s, reinterpret_cast<const float2*>(uh),
                       reinterpret_cast<const float2*>(vh), reinterpret_cast<float2*>(what), mean, batch, nx, ny, my1,
                       (float)(2.0 * M_PI / Lx), (float)(2.0 * M_PI / Ly), (float)(1.0 / ((double)nx * ny)));
    return check_launch("spec_ns_init");
}

// The step of every entry point: ghat == NULL and drag == 0 launch the unforced kernels, that == NULL the unscalared ones, b == 0 the passive ones;
// st != NULL (amp, key, clock, ids; its sqdt is set here) takes the forced path, with or without ghat and drag, and kicks after every step;
// lin != NULL takes the forced path too, with the table's factors in stages 1-3 (nu and drag are then unused: the table holds them).
// dwhat != NULL (never with that): the tangent-linear step, the same launches in their TANGENT forms on the tangent layout of work; the choice
// of the base's kernels is the one made without dwhat, so what comes out bitwise as from that call.  ntan >= 1 (with dwhat, no dghat): dwhat holds
// ntan tangents [ntan][B][my1][nx] on that one base, the TANGENTS forms on the layout of ntan tangents; ntan == 0: the one tangent's call.
// dthat != NULL (with that and dwhat, ntan == 0): the tangent of the scalar system, (dw^, dtheta^) in the launches of the scalar step on the
// 20-field layout; (what, that) come out bitwise as from the call without the perturbation.  dthat != NULL with ntan >= 1 (no dghat): ntan pairs
// (dwhat, dthat) [ntan][B][my1][nx] on the one base (w^, theta^), the TANSCS forms on the layout of 10 + 10 ntan fields.
static int spec_ns_step(const char* who, float* what, float* that, const float* mean, const float* ghat, int gbatch, void* work,
                        size_t work_bytes_, int batch, int nx, int ny, double Lx, double Ly, double dt, double nu, double drag, double kappa,
                        double gx, double gy, double bx, double by, int nsteps, void* stream, const PsStoch* st = nullptr,
                        const float* lin = nullptr, float* dwhat = nullptr, const float* dghat = nullptr, int dgbatch = 0,
                        int ntan = 0, float* dthat = nullptr) {
    if (!what || !mean || !work || batch < 1) return fail(NNS_ERR_INVALID_ARG, "%s: NULL pointer or batch < 1", who);
    if (dwhat && that && !dthat) return fail(NNS_ERR_UNSUPPORTED, "%s: the tangent of the scalar system is not built", who);
    if (int rc = check_step_numbers(who, dt, nu, drag, nsteps)) return rc;
    if (int rc = check_scalar_numbers(who, kappa, gx, gy)) return rc;
    if (int rc = check_buoyancy(who, bx, by)) return rc;
    if (int rc = check_gbatch(who, ghat, gbatch, batch)) return rc;
    if (dghat ? (dgbatch != 1 && dgbatch != batch) : dgbatch != 0)
        return fail(NNS_ERR_INVALID_ARG, "%s: dgbatch = %d must be 0 without dghat, 1 or batch = %d with it", who, dgbatch, batch);
    if (int rc = check_common(who, batch, nx, ny, Lx, Ly, work_bytes_, ntan && dthat ? kWorkScalarTangents : ntan ? kWorkTangents : dthat ? kWorkScalarTangent : dwhat ? kWorkTangent : that ? kWorkScalar : kWorkFlow, ntan)) return rc;
    if (nsteps == 0) return NNS_OK;
    hipStream_t s = as_stream(stream);
    float2* W = reinterpret_cast<float2*>(what);
    const PsWork L(work, batch, nx, ny, ntan && dthat ? scalar_tangents_layout(ntan) : ntan ? tangents_layout(ntan) : dthat ? kLayScalarTangent : dwhat ? kLayTangent : that ? kLayScalar : kLayFlow, Lx, Ly, (float)(-0.5 * nu * dt), (float)dt);
    const PsTangent tangent{reinterpret_cast<float2*>(dwhat), dthat ? L.A + 2 * L.col.fstride : L.At, reinterpret_cast<const float2*>(dghat), dgbatch == 1 && batch > 1 ? 1 : 0};
    const PsTangent* tg = dwhat && !ntan ? &tangent : nullptr;
    const PsTangentScalar tanscalar{reinterpret_cast<float2*>(dthat), L.A + 3 * L.col.fstride};      // the scalar system's: A, A_theta, dA, dA_theta
    const PsTangentScalar* tt = dthat && !ntan ? &tanscalar : nullptr;
    const PsTangents tangents{reinterpret_cast<float2*>(dwhat), dthat ? L.A + 2 * L.col.fstride : L.At, L.col.fstride, ntan};      // dA[k] follows A (with a scalar: A_theta), a field apart like the members
    const PsTangents* ts = ntan ? &tangents : nullptr;
    const PsTangentsScalar tanscalars{reinterpret_cast<float2*>(dthat), L.A + (size_t)(2 + ntan) * L.col.fstride};      // dA_theta[k] follows dA[K]
    const PsTangentsScalar* tu = dthat && ntan ? &tanscalars : nullptr;
    const PsForce force{reinterpret_cast<const float2*>(ghat), gbatch == 1 && batch > 1 ? 1 : 0, (float)(0.5 * drag * dt)};
    const PsForce* fc = ghat || drag > 0 || st || lin ? &force : nullptr;
    const PsLinear linear{reinterpret_cast<const float2*>(lin)};
    const PsLinear* li = lin ? &linear : nullptr;
    PsStoch stoch{};
    if (st) {
        stoch = *st;
        stoch.sqdt = (float)std::sqrt(dt);
    }
    const PsStoch* stc = st ? &stoch : nullptr;
    const PsScalar scalar{reinterpret_cast<float2*>(that), L.At, (float)(-0.5 * kappa * dt)};
    const PsGrad grad{(float)gx, (float)gy};
    const PsScalar* sc = that ? &scalar : nullptr;
    const PsBuoyGrad buoy{(float)gx, (float)gy, (float)(-(double)ny * by), (float)((double)ny * bx)};
    const PsBuoyGrad* bu = that && (bx != 0.0 || by != 0.0) ? &buoy : nullptr;
    auto col = [&](int S, int emit) {
        return dispatch_pow2(nx, "spec_ns", [&](auto n) { return launch_col_stage<decltype(n)::value>(S, L.Ph, L.G, W, L.A, mean, L.col, emit, fc, sc, s, stc, li, tg, ts, tt, tu); });
    };
    auto row = [&]() {
        return dispatch_pow2(ny, "spec_ns", [&](auto n) {
            constexpr int N = decltype(n)::value;
            if (tu) return ps_scalar_tangents_row(N, L.G, L.Ph, &L.row, s, bu ? (const void*)bu : (const void*)&grad, bu != nullptr, ntan);
            if (ts) return launch_row_tans<N>(L.G, L.Ph, L.row, ntan, s);
            if (tt) return ps_scalar_tangent_row(N, L.G, L.Ph, &L.row, s, bu ? (const void*)bu : (const void*)&grad, bu != nullptr);
            if (tg) return launch_row_tan<N>(L.G, L.Ph, L.row, s);
            return bu ? launch_row<N>(L.G, L.Ph, L.row, s, *bu) : that ? launch_row<N>(L.G, L.Ph, L.row, s, grad) : launch_row<N>(L.G, L.Ph, L.row, s);
        });
    };
    if (int rc = col(0, 1)) return rc;
    for (int k = 0; k < nsteps; ++k) {
        for (int S = 1; S <= 4; ++S) {
            if (int rc = row()) return rc;
            if (int rc = col(S, k + 1 < nsteps)) return rc;
        }
    }
    return NNS_OK;
}

NNS_API int nns_spec_ns_step_f32(float* what, const float* mean, void* work, size_t work_bytes_, int batch, int nx, int ny, double Lx,
                                 double Ly, double dt, double nu, int nsteps, void* stream) {
    return spec_ns_step("spec_ns_step", what, nullptr, mean, nullptr, 0, work, work_bytes_, batch, nx, ny, Lx, Ly, dt, nu, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0,
                        nsteps, stream);
}

NNS_API int nns_spec_ns_step_forced_f32(float* what, const float* mean, const float* ghat, int gbatch, void* work, size_t work_bytes_,
                                        int batch, int nx, int ny, double Lx, double Ly, double dt, double nu, double drag, int nsteps,
                                        void* stream) {
    return spec_ns_step("spec_ns_step_forced", what, nullptr, mean, ghat, gbatch, work, work_bytes_, batch, nx, ny, Lx, Ly, dt, nu, drag, 0.0, 0.0,
                        0.0, 0.0, 0.0, nsteps, stream);
}

NNS_API int nns_spec_ns_step_scalar_f32(float* what, float* that, const float* mean, const float* ghat, int gbatch, void* work,
                                        size_t work_bytes_, int batch, int nx, int ny, double Lx, double Ly, double dt, double nu, double drag,
                                        double kappa, double gx, double gy, int nsteps, void* stream) {
    if (!that) return fail(NNS_ERR_INVALID_ARG, "spec_ns_step_scalar: NULL pointer or batch < 1");
    return spec_ns_step("spec_ns_step_scalar", what, that, mean, ghat, gbatch, work, work_bytes_, batch, nx, ny, Lx, Ly, dt, nu, drag, kappa, gx,
                        gy, 0.0, 0.0, nsteps, stream);
}

NNS_API int nns_spec_ns_step_buoyant_f32(float* what, float* that, const float* mean, const float* ghat, int gbatch, void* work,
                                         size_t work_bytes_, int batch, int nx, int ny, double Lx, double Ly, double dt, double nu, double drag,
                                         double kappa, double gx, double gy, double bx, double by, int nsteps, void* stream) {
    if (!that) return fail(NNS_ERR_INVALID_ARG, "spec_ns_step_buoyant: NULL pointer or batch < 1");
    return spec_ns_step("spec_ns_step_buoyant", what, that, mean, ghat, gbatch, work, work_bytes_, batch, nx, ny, Lx, Ly, dt, nu, drag, kappa, gx,
                        gy, bx, by, nsteps, stream);
}

NNS_API int nns_spec_ns_step_stochastic_f32(float* what, float* that, const float* mean, const float* ghat, int gbatch, void* work,
                                            size_t work_bytes_, int batch, int nx, int ny, double Lx, double Ly, double dt, double nu, double drag,
                                            double kappa, double gx, double gy, double bx, double by, const float* amp, unsigned long long seed,
                                            long long* clock, const int* ids, int nsteps, void* stream) {
    if (!amp || !clock || !ids) return fail(NNS_ERR_INVALID_ARG, "spec_ns_step_stochastic: amp, clock and ids must be non-NULL");
    const PsStoch st{amp, (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), clock, ids, 0.f};
    return spec_ns_step("spec_ns_step_stochastic", what, that, mean, ghat, gbatch, work, work_bytes_, batch, nx, ny, Lx, Ly, dt, nu, drag,
                        that ? kappa : 0.0, that ? gx : 0.0, that ? gy : 0.0, that ? bx : 0.0, that ? by : 0.0, nsteps, stream, &st);
}

NNS_API int nns_spec_ns_step_linear_f32(float* what, float* that, const float* mean, const float* ghat, int gbatch, void* work, size_t work_bytes_,
                                        int batch, int nx, int ny, double Lx, double Ly, double dt, double kappa, double gx, double gy, double bx,
                                        double by, const float* lin, const float* amp, unsigned long long seed, long long* clock, const int* ids,
                                        int nsteps, void* stream) {
    if (!lin) return fail(NNS_ERR_INVALID_ARG, "spec_ns_step_linear: lin must be non-NULL");
    const bool noise = amp && clock && ids;
    if (!noise && (amp || clock || ids))
        return fail(NNS_ERR_INVALID_ARG, "spec_ns_step_linear: amp, clock and ids must be all NULL (no noise) or all non-NULL");
    const PsStoch st{amp, (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), clock, ids, 0.f};
    return spec_ns_step("spec_ns_step_linear", what, that, mean, ghat, gbatch, work, work_bytes_, batch, nx, ny, Lx, Ly, dt, 0.0, 0.0,
                        that ? kappa : 0.0, that ? gx : 0.0, that ? gy : 0.0, that ? bx : 0.0, that ? by : 0.0, nsteps, stream,
                        noise ? &st : nullptr, lin);
}

NNS_API int nns_spec_ns_tangent_workspace(int batch, int nx, int ny, size_t* bytes) {
    if (!bytes || batch < 1) return fail(NNS_ERR_INVALID_ARG, "spec_ns_tangent_workspace: bytes must be non-NULL and batch >= 1 (batch = %d)", batch);
    if (int rc = check_axes("spec_ns_tangent_workspace", nx, ny)) return rc;
    *bytes = tangent_work_bytes(batch, nx, ny);
    return NNS_OK;
}

NNS_API int nns_spec_ns_step_tangent_f32(float* what, float* dwhat, const float* mean, const float* ghat, int gbatch, const float* dghat,
                                         int dgbatch, void* work, size_t work_bytes_, int batch, int nx, int ny, double Lx, double Ly, double dt,
                                         double nu, double drag, const float* lin, const float* amp, unsigned long long seed, long long* clock,
                                         const int* ids, int nsteps, void* stream) {
    if (!dwhat) return fail(NNS_ERR_INVALID_ARG, "spec_ns_step_tangent: dwhat must be non-NULL");
    const bool noise = amp && clock && ids;
    if (!noise && (amp || clock || ids))
        return fail(NNS_ERR_INVALID_ARG, "spec_ns_step_tangent: amp, clock and ids must be all NULL (no noise) or all non-NULL");
    const PsStoch st{amp, (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), clock, ids, 0.f};
    return spec_ns_step("spec_ns_step_tangent", what, nullptr, mean, ghat, gbatch, work, work_bytes_, batch, nx, ny, Lx, Ly, dt, lin ? 0.0 : nu,
                        lin ? 0.0 : drag, 0.0, 0.0, 0.0, 0.0, 0.0, nsteps, stream, noise ? &st : nullptr, lin, dwhat, dghat, dgbatch);
}

NNS_API int nns_spec_ns_scalar_tangent_workspace(int batch, int nx, int ny, size_t* bytes) {
    if (!bytes || batch < 1) return fail(NNS_ERR_INVALID_ARG, "spec_ns_scalar_tangent_workspace: bytes must be non-NULL and batch >= 1 (batch = %d)", batch);
    if (int rc = check_axes("spec_ns_scalar_tangent_workspace", nx, ny)) return rc;
    *bytes = scalar_tangent_work_bytes(batch, nx, ny);
    return NNS_OK;
}

// The base's kernels are chosen as ops.spec_ns_advance_ chooses its entry: lin the linear step's (nu and drag sit in the table), amp / clock / ids
// the stochastic one's, b != 0 the buoyant one's, else the scalar one's.
NNS_API int nns_spec_ns_step_scalar_tangent_f32(float* what, float* that, float* dwhat, float* dthat, const float* mean, const float* ghat,
                                                int gbatch, const float* dghat, int dgbatch, void* work, size_t work_bytes_, int batch, int nx,
                                                int ny, double Lx, double Ly, double dt, double nu, double drag, double kappa, double gx,
                                                double gy, double bx, double by, const float* lin, const float* amp, unsigned long long seed,
                                                long long* clock, const int* ids, int nsteps, void* stream) {
    if (!that || !dwhat || !dthat) return fail(NNS_ERR_INVALID_ARG, "spec_ns_step_scalar_tangent: that, dwhat and dthat must be non-NULL");
    const bool noise = amp && clock && ids;
    if (!noise && (amp || clock || ids))
        return fail(NNS_ERR_INVALID_ARG, "spec_ns_step_scalar_tangent: amp, clock and ids must be all NULL (no noise) or all non-NULL");
    const PsStoch st{amp, (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), clock, ids, 0.f};
    return spec_ns_step("spec_ns_step_scalar_tangent", what, that, mean, ghat, gbatch, work, work_bytes_, batch, nx, ny, Lx, Ly, dt,
                        lin ? 0.0 : nu, lin ? 0.0 : drag, kappa, gx, gy, bx, by, nsteps, stream, noise ? &st : nullptr, lin, dwhat, dghat, dgbatch,
                        0, dthat);
}

NNS_API int nns_spec_ns_tangents_workspace(int batch, int ntan, int nx, int ny, size_t* bytes) {
    if (!bytes || batch < 1) return fail(NNS_ERR_INVALID_ARG, "spec_ns_tangents_workspace: bytes must be non-NULL and batch >= 1 (batch = %d)", batch);
    if (ntan < 1 || ntan > kMaxTangents) return fail(NNS_ERR_INVALID_ARG, "spec_ns_tangents_workspace: ntan = %d must be in [1, %d]", ntan, kMaxTangents);
    if (int rc = check_axes("spec_ns_tangents_workspace", nx, ny)) return rc;
    *bytes = tangents_work_bytes(batch, ntan, nx, ny);
    return NNS_OK;
}

NNS_API int nns_spec_ns_step_tangents_f32(float* what, float* dwhat, int ntan, const float* mean, const float* ghat, int gbatch, void* work,
                                          size_t work_bytes_, int batch, int nx, int ny, double Lx, double Ly, double dt, double nu, double drag,
                                          const float* lin, const float* amp, unsigned long long seed, long long* clock, const int* ids,
                                          int nsteps, void* stream) {
    if (!dwhat) return fail(NNS_ERR_INVALID_ARG, "spec_ns_step_tangents: dwhat must be non-NULL");
    if (ntan < 1 || ntan > kMaxTangents) return fail(NNS_ERR_INVALID_ARG, "spec_ns_step_tangents: ntan = %d must be in [1, %d]", ntan, kMaxTangents);
    const bool noise = amp && clock && ids;
    if (!noise && (amp || clock || ids))
        return fail(NNS_ERR_INVALID_ARG, "spec_ns_step_tangents: amp, clock and ids must be all NULL (no noise) or all non-NULL");
    const PsStoch st{amp, (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), clock, ids, 0.f};
    return spec_ns_step("spec_ns_step_tangents", what, nullptr, mean, ghat, gbatch, work, work_bytes_, batch, nx, ny, Lx, Ly, dt, lin ? 0.0 : nu,
                        lin ? 0.0 : drag, 0.0, 0.0, 0.0, 0.0, 0.0, nsteps, stream, noise ? &st : nullptr, lin, dwhat, nullptr, 0, ntan);
}

NNS_API int nns_spec_ns_scalar_tangents_workspace(int batch, int ntan, int nx, int ny, size_t* bytes) {
    if (!bytes || batch < 1) return fail(NNS_ERR_INVALID_ARG, "spec_ns_scalar_tangents_workspace: bytes must be non-NULL and batch >= 1 (batch = %d)", batch);
    if (ntan < 1 || ntan > kMaxTangents) return fail(NNS_ERR_INVALID_ARG, "spec_ns_scalar_tangents_workspace: ntan = %d must be in [1, %d]", ntan, kMaxTangents);
    if (int rc = check_axes("spec_ns_scalar_tangents_workspace", nx, ny)) return rc;
    *bytes = scalar_tangents_work_bytes(batch, ntan, nx, ny);
    return NNS_OK;
}

// The base's kernels are chosen as in nns_spec_ns_step_scalar_tangent_f32; every member pair is that call's with dghat = NULL.
NNS_API int nns_spec_ns_step_scalar_tangents_f32(float* what, float* that, float* dwhat, float* dthat, int ntan, const float* mean,
                                                 const float* ghat, int gbatch, void* work, size_t work_bytes_, int batch, int nx, int ny,
                                                 double Lx, double Ly, double dt, double nu, double drag, double kappa, double gx, double gy,
                                                 double bx, double by, const float* lin, const float* amp, unsigned long long seed,
                                                 long long* clock, const int* ids, int nsteps, void* stream) {
    if (!that || !dwhat || !dthat) return fail(NNS_ERR_INVALID_ARG, "spec_ns_step_scalar_tangents: that, dwhat and dthat must be non-NULL");
    if (ntan < 1 || ntan > kMaxTangents) return fail(NNS_ERR_INVALID_ARG, "spec_ns_step_scalar_tangents: ntan = %d must be in [1, %d]", ntan, kMaxTangents);
    const bool noise = amp && clock && ids;
    if (!noise && (amp || clock || ids))
        return fail(NNS_ERR_INVALID_ARG, "spec_ns_step_scalar_tangents: amp, clock and ids must be all NULL (no noise) or all non-NULL");
    const PsStoch st{amp, (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), clock, ids, 0.f};
    return spec_ns_step("spec_ns_step_scalar_tangents", what, that, mean, ghat, gbatch, work, work_bytes_, batch, nx, ny, Lx, Ly, dt,
                        lin ? 0.0 : nu, lin ? 0.0 : drag, kappa, gx, gy, bx, by, nsteps, stream, noise ? &st : nullptr, lin, dwhat, nullptr, 0, ntan,
                        dthat);
}

// dwhat, ntan, batch and the box of the Gram and the combine call
static int check_tangents(const char* who, const void* dwhat, const void* other, int ntan, int batch, int nx, int ny) {
    if (!dwhat || !other || batch < 1) return fail(NNS_ERR_INVALID_ARG, "%s: NULL pointer or batch < 1", who);
    if (ntan < 1 || ntan > kMaxTangents) return fail(NNS_ERR_INVALID_ARG, "%s: ntan = %d must be in [1, %d]", who, ntan, kMaxTangents);
    return check_axes(who, nx, ny);
}

NNS_API int nns_spec_ns_tangent_gram_f64(const float* dwhat, int ntan, double* out, int batch, int nx, int ny, double Lx, double Ly, void* stream) {
    if (int rc = check_tangents("spec_ns_tangent_gram", dwhat, out, ntan, batch, nx, ny)) return rc;
    if (int rc = check_lengths("spec_ns_tangent_gram", Lx, Ly)) return rc;
    const int my1 = kept_y(ny);
    const double n = (double)nx * ny;
    hipLaunchKernelGGL(ps_tangent_gram_kernel, dim3(ntan * (ntan + 1) / 2, batch), dim3(kDiagT), 0, as_stream(stream),
                       reinterpret_cast<const float2*>(dwhat), out, ntan, (long)batch * my1 * nx, nx, my1, 2.0 * M_PI / Lx, 2.0 * M_PI / Ly, 1.0 / (n * n));
    return check_launch("spec_ns_tangent_gram");
}

NNS_API int nns_spec_ns_tangent_combine_f32(float* dwhat, int ntan, const double* coef, int batch, int nx, int ny, void* stream) {
    if (int rc = check_tangents("spec_ns_tangent_combine", dwhat, coef, ntan, batch, nx, ny)) return rc;
    const long per = (long)kept_y(ny) * nx;
    hipLaunchKernelGGL(ps_tangent_combine_kernel, dim3(capped_grid((per + 255) / 256, 4096), batch), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<float2*>(dwhat), coef, ntan, (long)batch * per, per);
    return check_launch("spec_ns_tangent_combine");
}

NNS_API int nns_spec_ns_adjoint_workspace(int batch, int nx, int ny, size_t* bytes) {
    if (!bytes || batch < 1) return fail(NNS_ERR_INVALID_ARG, "spec_ns_adjoint_workspace: bytes must be non-NULL and batch >= 1 (batch = %d)", batch);
    if (int rc = check_axes("spec_ns_adjoint_workspace", nx, ny)) return rc;
    *bytes = adjoint_work_bytes(batch, nx, ny);
    return NNS_OK;
}

// The reverse mode of spec_ns_step's steady forms, last step first; that0 == NULL: the forced flow's, else the scalar's and the buoyant one's
// (b != 0), the scalar riding in the flow adjoint's launches.  Per step: the stage states s1, s2, s3 (of w^, and of theta^) recomputed from the
// step's saved start spectra by the forward's own launches (stage 0, then three row / column pairs whose column kernels also store the next
// stage's input: 7), then the adjoint's stage 4 column launch and four row / column pairs (9).  No allocation, no host synchronisation.
// lin != NULL: the linear step's (nu and drag are then unused: the table holds them); the recomputation's stages 1-3 are the LINEAR kernels with
// the stage store and the adjoint's stages 3-1 the LINEAR adjoint kernels, the other launches are those of the forced step.  A stochastic step
// needs no form of its own: its start spectra carry the kicks, whose Jacobian is the identity.  lbar != NULL (with lin): the adjoint's stages 3-1
// are the OPERATOR kernels, which also sum the table's cotangent; the launches, the workspace and everything else are the same.
static int spec_ns_step_adjoint(const char* who, const float* what0, const float* that0, const float* mean, const float* ghat, int gbatch,
                                float* lam, float* mu, float* gbar, void* work, size_t work_bytes_, int batch, int nx, int ny, double Lx,
                                double Ly, double dt, double nu, double drag, double kappa, double gx, double gy, double bx, double by,
                                int nsteps, void* stream, const float* lin = nullptr, float* lbar = nullptr) {
    const bool scalar = that0 != nullptr;
    if (!what0 || !mean || !lam || !work || batch < 1) return fail(NNS_ERR_INVALID_ARG, "%s: NULL pointer or batch < 1", who);
    if (int rc = check_step_numbers(who, dt, nu, drag, nsteps)) return rc;
    if (int rc = check_scalar_numbers(who, kappa, gx, gy)) return rc;
    if (int rc = check_buoyancy(who, bx, by)) return rc;
    if (int rc = check_gbatch(who, ghat, gbatch, batch)) return rc;
    if (int rc = check_common(who, batch, nx, ny, Lx, Ly, work_bytes_, scalar ? kWorkScalarAdjoint : kWorkAdjoint)) return rc;
    hipStream_t s = as_stream(stream);
    if (nsteps == 0) {
        const long zbytes = (long)((size_t)batch * kept_y(ny) * nx * sizeof(float2));
        void* zb[2] = {gbar ? gbar : lbar, lbar};
        const long zn[2] = {zbytes, zbytes};
        const int nz = (gbar ? 1 : 0) + (lbar ? 1 : 0);
        return nz ? zero_buffers(zb, zn, nz, s) : NNS_OK;
    }
    const PsWork L(work, batch, nx, ny, scalar ? kLayScalarAdjoint : kLayAdjoint, Lx, Ly, (float)(-0.5 * nu * dt), (float)dt);
    const long fstride = L.col.fstride;
    float2* wstages = L.keep;                                                                  // s1, s2, s3 of w^
    float2* tstages = scalar ? wstages + 3 * fstride : nullptr;                                // and of theta^
    const PsForce force{reinterpret_cast<const float2*>(ghat), gbatch == 1 && batch > 1 ? 1 : 0, (float)(0.5 * drag * dt)};
    const PsForce* fc = ghat || drag > 0 || lin ? &force : nullptr;                            // the forward's choice of kernels: its bits
    const PsLinear linear{reinterpret_cast<const float2*>(lin)};
    const PsLinear* li = lin ? &linear : nullptr;
    const float hkdt = (float)(-0.5 * kappa * dt);
    const PsGrad grad{(float)gx, (float)gy};
    const PsBuoyGrad buoy{(float)gx, (float)gy, (float)(-(double)ny * by), (float)((double)ny * bx)};
    const bool buoyant = scalar && (bx != 0.0 || by != 0.0);
    const PsAdjGrad agrad{(float)gx, (float)gy, (float)bx, (float)by};
    // wbar and thetabar take the accumulators' places (PsLayout's note): the recomputation is over when adjoint stage 3 first writes them
    PsAdjScalar ad{PsAdj{reinterpret_cast<float2*>(lam), scalar ? L.A : L.At, reinterpret_cast<float2*>(gbar), nullptr, force.hdrag, 0},
                   reinterpret_cast<float2*>(mu), L.At, nullptr, hkdt};
    auto row = [&]() {
        return dispatch_pow2(ny, "spec_ns", [&](auto n) {
            constexpr int N = decltype(n)::value;
            return buoyant ? launch_row<N>(L.G, L.Ph, L.row, s, buoy) : scalar ? launch_row<N>(L.G, L.Ph, L.row, s, grad) : launch_row<N>(L.G, L.Ph, L.row, s);
        });
    };
    auto row_adj = [&]() {
        return dispatch_pow2(ny, "spec_ns", [&](auto n) {
            constexpr int N = decltype(n)::value;
            return scalar ? launch_row_adj<N>(L.G, L.Ph, L.row, s, agrad) : launch_row_adj<N>(L.G, L.Ph, L.row, s);
        });
    };
    for (int k = nsteps - 1; k >= 0; --k) {
        float2* W = const_cast<float2*>(reinterpret_cast<const float2*>(what0)) + (size_t)k * fstride;      // stages 0-3 only read W and T
        float2* T = scalar ? const_cast<float2*>(reinterpret_cast<const float2*>(that0)) + (size_t)k * fstride : nullptr;
        const PsScalar sc{T, L.At, hkdt};
        if (int rc = dispatch_pow2(nx, "spec_ns", [&](auto n) {
                return launch_col_stage<decltype(n)::value>(0, L.Ph, L.G, W, L.A, mean, L.col, 1, nullptr, scalar ? &sc : nullptr, s);
            }))
            return rc;
        for (int S = 1; S <= 3; ++S) {
            if (int rc = row()) return rc;
            const size_t off = (size_t)(S - 1) * fstride;
            if (int rc = dispatch_pow2(nx, "spec_ns", [&](auto n) {
                    constexpr int N = decltype(n)::value;
                    return scalar ? launch_col_keep<N>(S, L.Ph, L.G, W, L.A, mean, L.col, fc, li, s, PsKeepScalar{wstages + off, tstages + off}, sc)
                                  : launch_col_keep<N>(S, L.Ph, L.G, W, L.A, mean, L.col, fc, li, s, PsKeep{wstages + off});
                }))
                return rc;
        }
        for (int S = 4; S >= 0; --S) {
            if (S < 4)
                if (int rc = row_adj()) return rc;
            ad.state = S >= 2 ? wstages + (size_t)(S - 2) * fstride : W;
            ad.tstate = scalar && S >= 2 ? tstages + (size_t)(S - 2) * fstride : T;
            ad.ginit = k == nsteps - 1;
            if (int rc = dispatch_pow2(nx, "spec_ns", [&](auto n) {
                    constexpr int N = decltype(n)::value;
                    if (li && lbar && S >= 1 && S <= 3) {                    // the state this stage's r belongs to, and the step's start
                        float2* lb = reinterpret_cast<float2*>(lbar);
                        // the step's own sum lives in a field these stages leave idle: the flow's accumulator A (its wbar is in A_theta's
                        // place), with a scalar theta^'s s3 (read by stage 4 alone, stored again by the next step's recomputation)
                        float2* lstep = scalar ? tstages + 2 * fstride : L.A;
                        const float2* own = wstages + (size_t)(S - 1) * fstride;
                        return scalar ? launch_col_adj<N>(S, L.Ph, L.G, mean, L.col, PsAdjScalarOperator{PsAdjScalarLinear{ad, li->lin}, lb, lstep, own, W}, s)
                                      : launch_col_adj<N>(S, L.Ph, L.G, mean, L.col, PsAdjOperator{PsAdjLinear{ad, li->lin}, lb, lstep, own, W}, s);
                    }
                    if (li && S >= 1 && S <= 3)
                        return scalar ? launch_col_adj<N>(S, L.Ph, L.G, mean, L.col, PsAdjScalarLinear{ad, li->lin}, s)
                                      : launch_col_adj<N>(S, L.Ph, L.G, mean, L.col, PsAdjLinear{ad, li->lin}, s);
                    return scalar ? launch_col_adj<N>(S, L.Ph, L.G, mean, L.col, ad, s) : launch_col_adj<N, PsAdj>(S, L.Ph, L.G, mean, L.col, ad, s);
                }))
                return rc;
        }
    }
    return NNS_OK;
}

NNS_API int nns_spec_ns_step_adjoint_f32(const float* what0, const float* mean, const float* ghat, int gbatch, float* lam, float* gbar, void* work,
                                         size_t work_bytes_, int batch, int nx, int ny, double Lx, double Ly, double dt, double nu, double drag,
                                         int nsteps, void* stream) {
    return spec_ns_step_adjoint("spec_ns_step_adjoint", what0, nullptr, mean, ghat, gbatch, lam, nullptr, gbar, work, work_bytes_, batch, nx, ny, Lx,
                                Ly, dt, nu, drag, 0.0, 0.0, 0.0, 0.0, 0.0, nsteps, stream);
}

NNS_API int nns_spec_ns_scalar_adjoint_workspace(int batch, int nx, int ny, size_t* bytes) {
    if (!bytes || batch < 1)
        return fail(NNS_ERR_INVALID_ARG, "spec_ns_scalar_adjoint_workspace: bytes must be non-NULL and batch >= 1 (batch = %d)", batch);
    if (int rc = check_axes("spec_ns_scalar_adjoint_workspace", nx, ny)) return rc;
    *bytes = scalar_adjoint_work_bytes(batch, nx, ny);
    return NNS_OK;
}

NNS_API int nns_spec_ns_step_scalar_adjoint_f32(const float* what0, const float* that0, const float* mean, const float* ghat, int gbatch,
                                                float* lam, float* mu, float* gbar, void* work, size_t work_bytes_, int batch, int nx, int ny,
                                                double Lx, double Ly, double dt, double nu, double drag, double kappa, double gx, double gy,
                                                double bx, double by, int nsteps, void* stream) {
    if (!that0 || !mu) return fail(NNS_ERR_INVALID_ARG, "spec_ns_step_scalar_adjoint: NULL pointer or batch < 1");
    return spec_ns_step_adjoint("spec_ns_step_scalar_adjoint", what0, that0, mean, ghat, gbatch, lam, mu, gbar, work, work_bytes_, batch, nx, ny,
                                Lx, Ly, dt, nu, drag, kappa, gx, gy, bx, by, nsteps, stream);
}

NNS_API int nns_spec_ns_step_linear_adjoint_f32(const float* what0, const float* that0, const float* mean, const float* ghat, int gbatch,
                                                float* lam, float* mu, float* gbar, void* work, size_t work_bytes_, int batch, int nx, int ny,
                                                double Lx, double Ly, double dt, double kappa, double gx, double gy, double bx, double by,
                                                const float* lin, int nsteps, void* stream) {
    if (!lin) return fail(NNS_ERR_INVALID_ARG, "spec_ns_step_linear_adjoint: lin must be non-NULL");
    if (!that0 != !mu) return fail(NNS_ERR_INVALID_ARG, "spec_ns_step_linear_adjoint: that0 and mu must be both NULL (no scalar) or both non-NULL");
    return spec_ns_step_adjoint("spec_ns_step_linear_adjoint", what0, that0, mean, ghat, gbatch, lam, mu, gbar, work, work_bytes_, batch, nx, ny,
                                Lx, Ly, dt, 0.0, 0.0, that0 ? kappa : 0.0, that0 ? gx : 0.0, that0 ? gy : 0.0, that0 ? bx : 0.0, that0 ? by : 0.0,
                                nsteps, stream, lin);
}

NNS_API int nns_spec_ns_step_operator_adjoint_f32(const float* what0, const float* that0, const float* mean, const float* ghat, int gbatch,
                                                  float* lam, float* mu, float* gbar, void* work, size_t work_bytes_, int batch, int nx, int ny,
                                                  double Lx, double Ly, double dt, double kappa, double gx, double gy, double bx, double by,
                                                  const float* lin, int nsteps, void* stream, float* lbar) {
    if (!lin) return fail(NNS_ERR_INVALID_ARG, "spec_ns_step_operator_adjoint: lin must be non-NULL");
    if (!that0 != !mu) return fail(NNS_ERR_INVALID_ARG, "spec_ns_step_operator_adjoint: that0 and mu must be both NULL (no scalar) or both non-NULL");
    return spec_ns_step_adjoint("spec_ns_step_operator_adjoint", what0, that0, mean, ghat, gbatch, lam, mu, gbar, work, work_bytes_, batch, nx, ny,
                                Lx, Ly, dt, 0.0, 0.0, that0 ? kappa : 0.0, that0 ? gx : 0.0, that0 ? gy : 0.0, that0 ? bx : 0.0, that0 ? by : 0.0,
                                nsteps, stream, lin, lbar);
}

NNS_API int nns_spec_ns_second_adjoint_workspace(int batch, int nx, int ny, size_t* bytes) {
    if (!bytes || batch < 1)
        return fail(NNS_ERR_INVALID_ARG, "spec_ns_second_adjoint_workspace: bytes must be non-NULL and batch >= 1 (batch = %d)", batch);
    if (int rc = check_axes("spec_ns_second_adjoint_workspace", nx, ny)) return rc;
    *bytes = second_adjoint_work_bytes(batch, nx, ny);
    return NNS_OK;
}

// The second-order adjoint of the flow's steps, last step first: spec_ns_step_adjoint's sequence with a second quadruple riding in every launch.
// Per step: the stage states s1, s2, s3 and the tangent stages d1, d2, d3 recomputed from the step's saved (w^, dw^) by the tangent step's own
// launches (stage 0, then three row / column pairs whose column kernels carry the PsKeepTangent: 7), then the adjoint's stage 4 column launch and
// four ps_row_adj2_kernel / column pairs (9).  The base's kernels are chosen as spec_ns_step_adjoint chooses them (ghat, drag or lin: the forced
// forms), so lam and gbar are that call's bits.  No allocation, no host synchronisation.
NNS_API int nns_spec_ns_step_second_adjoint_f32(const float* what0, const float* dwhat0, const float* mean, const float* ghat, int gbatch,
                                                const float* dghat, int dgbatch, float* lam, float* dlam, float* gbar, float* dgbar, void* work,
                                                size_t work_bytes_, int batch, int nx, int ny, double Lx, double Ly, double dt, double nu,
                                                double drag, const float* lin, int nsteps, void* stream) {
    const char* who = "spec_ns_step_second_adjoint";
    if (!what0 || !mean || !lam || !work || batch < 1) return fail(NNS_ERR_INVALID_ARG, "%s: NULL pointer or batch < 1", who);
    if (!dwhat0 || !dlam) return fail(NNS_ERR_INVALID_ARG, "%s: dwhat0 and dlam must be non-NULL", who);
    if (lin) nu = drag = 0.0;                                                                  // the table holds them
    if (int rc = check_step_numbers(who, dt, nu, drag, nsteps)) return rc;
    if (int rc = check_gbatch(who, ghat, gbatch, batch)) return rc;
    if (dghat ? (dgbatch != 1 && dgbatch != batch) : dgbatch != 0)
        return fail(NNS_ERR_INVALID_ARG, "%s: dgbatch = %d must be 0 without dghat, 1 or batch = %d with it", who, dgbatch, batch);
    if (int rc = check_common(who, batch, nx, ny, Lx, Ly, work_bytes_, kWorkSecondAdjoint)) return rc;
    hipStream_t s = as_stream(stream);
    if (nsteps == 0) {
        const long zbytes = (long)((size_t)batch * kept_y(ny) * nx * sizeof(float2));
        void* zb[2] = {gbar ? gbar : dgbar, dgbar};
        const long zn[2] = {zbytes, zbytes};
        const int nz = (gbar ? 1 : 0) + (dgbar ? 1 : 0);
        return nz ? zero_buffers(zb, zn, nz, s) : NNS_OK;
    }
    const PsWork L(work, batch, nx, ny, kLaySecondAdjoint, Lx, Ly, (float)(-0.5 * nu * dt), (float)dt);
    const long fstride = L.col.fstride;
    float2* wstages = L.keep;                                                                  // s1, s2, s3 of w^
    float2* dstages = wstages + 3 * fstride;                                                   // d1, d2, d3 of dw^
    const PsForce force{reinterpret_cast<const float2*>(ghat), gbatch == 1 && batch > 1 ? 1 : 0, (float)(0.5 * drag * dt)};
    const PsForce* fc = ghat || drag > 0 || lin ? &force : nullptr;                            // the adjoint's choice of kernels: its bits
    const PsLinear linear{reinterpret_cast<const float2*>(lin)};
    const PsLinear* li = lin ? &linear : nullptr;
    // wbar and dwbar take the accumulators' places (PsLayout's note): the recomputation is over when adjoint stage 3 first writes them
    PsAdjSecond ad{PsAdj{reinterpret_cast<float2*>(lam), L.A, reinterpret_cast<float2*>(gbar), nullptr, force.hdrag, 0},
                   reinterpret_cast<float2*>(dlam), L.At, reinterpret_cast<float2*>(dgbar), nullptr};
    for (int k = nsteps - 1; k >= 0; --k) {
        float2* W = const_cast<float2*>(reinterpret_cast<const float2*>(what0)) + (size_t)k * fstride;      // stages 0-3 only read W and dW
        float2* dW = const_cast<float2*>(reinterpret_cast<const float2*>(dwhat0)) + (size_t)k * fstride;
        const PsTangent tg{dW, L.At, reinterpret_cast<const float2*>(dghat), dgbatch == 1 && batch > 1 ? 1 : 0};
        if (int rc = dispatch_pow2(nx, "spec_ns", [&](auto n) {
                return launch_col_stage<decltype(n)::value>(0, L.Ph, L.G, W, L.A, mean, L.col, 1, nullptr, nullptr, s, nullptr, nullptr, &tg);
            }))
            return rc;
        for (int S = 1; S <= 3; ++S) {
            if (int rc = dispatch_pow2(ny, "spec_ns", [&](auto n) { return launch_row_tan<decltype(n)::value>(L.G, L.Ph, L.row, s); })) return rc;
            const size_t off = (size_t)(S - 1) * fstride;
            const PsKeepTangent ke{wstages + off, dstages + off};
            if (int rc = ps_second_adjoint_col_keep(nx, S, L.Ph, L.G, W, L.A, mean, &L.col, fc, li, s, &tg, &ke)) return rc;
        }
        for (int S = 4; S >= 0; --S) {
            if (S < 4)
                if (int rc = ps_second_adjoint_row(ny, L.G, L.Ph, &L.row, s)) return rc;
            ad.state = S >= 2 ? wstages + (size_t)(S - 2) * fstride : W;
            ad.dstate = S >= 2 ? dstages + (size_t)(S - 2) * fstride : dW;
            ad.ginit = k == nsteps - 1;
            if (int rc = ps_second_adjoint_col(nx, S, L.Ph, L.G, mean, &L.col, &ad, lin, s)) return rc;
        }
    }
    return NNS_OK;
}

NNS_API int nns_spec_ns_scalar_workspace(int batch, int nx, int ny, size_t* bytes) {
    if (!bytes || batch < 1) return fail(NNS_ERR_INVALID_ARG, "spec_ns_scalar_workspace: bytes must be non-NULL and batch >= 1 (batch = %d)", batch);
    if (int rc = check_axes("spec_ns_scalar_workspace", nx, ny)) return rc;
    *bytes = scalar_work_bytes(batch, nx, ny);
    return NNS_OK;
}

NNS_API int nns_spec_ns_scalar_init_f32(const float* theta, float* that, void* work, size_t work_bytes_, int batch, int nx, int ny,
                                        void* stream) {
    if (!theta || !that || !work || batch < 1) return fail(NNS_ERR_INVALID_ARG, "spec_ns_scalar_init: NULL pointer or batch < 1");
    if (int rc = check_common("spec_ns_scalar_init", batch, nx, ny, 1.0, 1.0, work_bytes_, true)) return rc;
    float* th = static_cast<float*>(work);
    if (int rc = nns_spec_rfft2_f32(theta, th, batch, nx, ny, stream)) return rc;
    const int my1 = kept_y(ny);
    hipLaunchKernelGGL(ps_scalar_compact_kernel, dim3(pw_grid((long)batch * my1 * nx)), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const float2*>(th), reinterpret_cast<float2*>(that), batch, nx, ny, my1);
    return check_launch("spec_ns_scalar_init");
}

NNS_API int nns_spec_ns_scalar_field_f32(const float* that, float* theta, void* work, size_t work_bytes_, int batch, int nx, int ny,
                                         void* stream) {
    if (!that || !theta || !work || batch < 1) return fail(NNS_ERR_INVALID_ARG, "spec_ns_scalar_field: NULL pointer or batch < 1");
    if (int rc = check_common("spec_ns_scalar_field", batch, nx, ny, 1.0, 1.0, work_bytes_, true)) return rc;
    float* th = static_cast<float*>(work);
    hipLaunchKernelGGL(ps_scalar_expand_kernel, dim3(pw_grid((long)batch * nx * (ny / 2 + 1))), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const float2*>(that), reinterpret_cast<float2*>(th), batch, nx, ny, kept_y(ny));
    if (int rc = check_launch("spec_ns_scalar_field")) return rc;
    return nns_spec_irfft2_f32(th, theta, batch, nx, ny, stream);
}

NNS_API int nns_spec_ns_scalar_diag_f32(const float* what, const float* that, double* out, int batch, int nx, int ny, double Lx, double Ly,
                                        double kappa, void* stream) {
    if (!what || !that || !out || batch < 1) return fail(NNS_ERR_INVALID_ARG, "spec_ns_scalar_diag: NULL pointer or batch < 1");
    if (int rc = check_lengths("spec_ns_scalar_diag", Lx, Ly)) return rc;
    if (!(kappa >= 0) || !std::isfinite(kappa)) return fail(NNS_ERR_INVALID_ARG, "spec_ns_scalar_diag: kappa = %g must be finite and >= 0", kappa);
    if (int rc = check_axes("spec_ns_scalar_diag", nx, ny)) return rc;
    const double n = (double)nx * ny;
    hipLaunchKernelGGL(ps_scalar_diag_kernel, dim3(batch), dim3(kDiagT), 0, as_stream(stream), reinterpret_cast<const float2*>(what),
                       reinterpret_cast<const float2*>(that), out, nx, kept_y(ny), 2.0 * M_PI / Lx, 2.0 * M_PI / Ly, kappa, 1.0 / (n * n));
    return check_launch("spec_ns_scalar_diag");
}

NNS_API int nns_spec_ns_diag_f32(const float* what, const float* ghat, int gbatch, double* out, int batch, int nx, int ny, double Lx,
                                 double Ly, void* stream) {
    if (!what || !out || batch < 1) return fail(NNS_ERR_INVALID_ARG, "spec_ns_diag: NULL pointer or batch < 1");
    if (int rc = check_gbatch("spec_ns_diag", ghat, gbatch, batch)) return rc;
    if (int rc = check_box("spec_ns_diag", nx, ny, Lx, Ly)) return rc;
    const double n = (double)nx * ny;
    hipLaunchKernelGGL(ps_diag_kernel, dim3(batch), dim3(kDiagT), 0, as_stream(stream), reinterpret_cast<const float2*>(what),
                       reinterpret_cast<const float2*>(ghat), gbatch == 1 && batch > 1 ? 1 : 0, out, nx, kept_y(ny), 2.0 * M_PI / Lx,
                       2.0 * M_PI / Ly, 1.0 / (n * n));
    return check_launch("spec_ns_diag");
}

// The fields of both entry points: that == NULL or b == 0 end in the pressure kernel of the flow alone.
static int spec_ns_fields(const char* who, const float* what, const float* that, const float* mean, float* u, float* v, float* p, void* work,
                          size_t work_bytes_, int batch, int nx, int ny, double Lx, double Ly, double rho, double bx, double by, void* stream) {
    if (!what || !mean || !u || !v || !p || !work || batch < 1) return fail(NNS_ERR_INVALID_ARG, "%s: NULL pointer or batch < 1", who);
    if (!std::isfinite(rho)) return fail(NNS_ERR_INVALID_ARG, "%s: rho = %g must be finite", who, rho);
    if (int rc = check_buoyancy(who, bx, by)) return rc;
    if (int rc = check_common(who, batch, nx, ny, Lx, Ly, work_bytes_, that != nullptr)) return rc;
    hipStream_t s = as_stream(stream);
    const int my1 = kept_y(ny);
    const long nh = ny / 2 + 1, per = (long)batch * nx * nh, npts = (long)batch * nx * ny;
    float* spec = static_cast<float*>(work);                 // [6][B][nx][nh] complex: u_x, u_y, v_x, v_y, u, v
    float* phys = spec + 2 * 6 * per;                        // [4][B][nx][ny]: u_x, u_y, v_x, v_y; then q
    const float kx1 = (float)(2.0 * M_PI / Lx), ky1 = (float)(2.0 * M_PI / Ly);
    hipLaunchKernelGGL(ps_derivs_kernel, dim3(pw_grid(per)), dim3(256), 0, s, reinterpret_cast<const float2*>(what), mean,
                       reinterpret_cast<float2*>(spec), batch, nx, ny, my1, kx1, ky1);
    if (int rc = check_launch(who)) return rc;
    if (int rc = nns_spec_irfft2_f32(spec, phys, 4 * batch, nx, ny, stream)) return rc;
    if (int rc = nns_spec_irfft2_f32(spec + 2 * 4 * per, u, batch, nx, ny, stream)) return rc;
    if (int rc = nns_spec_irfft2_f32(spec + 2 * 5 * per, v, batch, nx, ny, stream)) return rc;
    hipLaunchKernelGGL(ps_source_kernel, dim3(pw_grid(npts)), dim3(256), 0, s, phys, phys, npts, (float)(2.0 * rho));
    if (int rc = check_launch(who)) return rc;
    if (int rc = nns_spec_rfft2_f32(phys, spec, batch, nx, ny, stream)) return rc;
    if (that && (bx != 0.0 || by != 0.0))
        hipLaunchKernelGGL(ps_pressure_buoyant_kernel, dim3(pw_grid(per)), dim3(256), 0, s, reinterpret_cast<float2*>(spec),
                           reinterpret_cast<const float2*>(that), batch, nx, ny, my1, kx1, ky1, (float)(rho * bx), (float)(rho * by));
    else
        hipLaunchKernelGGL(ps_pressure_kernel, dim3(pw_grid(per)), dim3(256), 0, s, reinterpret_cast<float2*>(spec), batch, nx, ny, kx1, ky1);
    if (int rc = check_launch(who)) return rc;
    return nns_spec_irfft2_f32(spec, p, batch, nx, ny, stream);
}

NNS_API int nns_spec_ns_fields_f32(const float* what, const float* mean, float* u, float* v, float* p, void* work, size_t work_bytes_,
                                   int batch, int nx, int ny, double Lx, double Ly, double rho, void* stream) {
    return spec_ns_fields("spec_ns_fields", what, nullptr, mean, u, v, p, work, work_bytes_, batch, nx, ny, Lx, Ly, rho, 0.0, 0.0, stream);
}

NNS_API int nns_spec_ns_fields_buoyant_f32(const float* what, const float* that, const float* mean, float* u, float* v, float* p, void* work,
                                           size_t work_bytes_, int batch, int nx, int ny, double Lx, double Ly, double rho, double bx, double by,
                                           void* stream) {
    if (!that) return fail(NNS_ERR_INVALID_ARG, "spec_ns_fields_buoyant: NULL pointer or batch < 1");
    return spec_ns_fields("spec_ns_fields_buoyant", what, that, mean, u, v, p, work, work_bytes_, batch, nx, ny, Lx, Ly, rho, bx, by, stream);
}

#elif defined(PSPEC_SCALAR_TANGENT_TU)      // the launches of the scalar system's tangent (declared at the head of this file)
int ps_scalar_tangent_col(int nx, int S, const void* Ph, void* G, void* W, void* A, const float* mean, const void* a, int emit, const void* fc,
                          const void* sc, void* stream, const void* st, const void* li, const void* tg, const void* tt) {
    return dispatch_pow2(nx, "spec_ns", [&](auto n) {
        return launch_col_stage<decltype(n)::value>(S, static_cast<const float2*>(Ph), static_cast<float2*>(G), static_cast<float2*>(W),
                                                    static_cast<float2*>(A), mean, *static_cast<const PsArgs*>(a), emit,
                                                    static_cast<const PsForce*>(fc), static_cast<const PsScalar*>(sc),
                                                    static_cast<hipStream_t>(stream), static_cast<const PsStoch*>(st),
                                                    static_cast<const PsLinear*>(li), static_cast<const PsTangent*>(tg), nullptr,
                                                    static_cast<const PsTangentScalar*>(tt));
    });
}

int ps_scalar_tangent_row(int ny, const void* G, void* Ph, const void* a, void* stream, const void* gr, int buoyant) {
    return dispatch_pow2(ny, "spec_ns", [&](auto n) {
        constexpr int N = decltype(n)::value;
        const float2* g = static_cast<const float2*>(G);
        float2* ph = static_cast<float2*>(Ph);
        const PsArgs& args = *static_cast<const PsArgs*>(a);
        hipStream_t s = static_cast<hipStream_t>(stream);
        return buoyant ? launch_row_tan_scalar<N>(g, ph, args, s, *static_cast<const PsBuoyGrad*>(gr))
                       : launch_row_tan_scalar<N>(g, ph, args, s, *static_cast<const PsGrad*>(gr));
    });
}
#elif defined(PSPEC_SECOND_ADJOINT_TU)      // the launches of the second-order adjoint (declared at the head of this file)
int ps_second_adjoint_col_keep(int nx, int S, const void* Ph, void* G, void* W, void* A, const float* mean, const void* a, const void* fc,
                               const void* li, void* stream, const void* tg, const void* ke) {
    return dispatch_pow2(nx, "spec_ns", [&](auto n) {
        return launch_col_keep<decltype(n)::value>(S, static_cast<const float2*>(Ph), static_cast<float2*>(G), static_cast<float2*>(W),
                                                   static_cast<float2*>(A), mean, *static_cast<const PsArgs*>(a), static_cast<const PsForce*>(fc),
                                                   static_cast<const PsLinear*>(li), static_cast<hipStream_t>(stream),
                                                   *static_cast<const PsKeepTangent*>(ke), *static_cast<const PsTangent*>(tg));
    });
}

int ps_second_adjoint_row(int ny, const void* G, void* Ph, const void* a, void* stream) {
    return dispatch_pow2(ny, "spec_ns", [&](auto n) {
        return launch_row_adj2<decltype(n)::value>(static_cast<const float2*>(G), static_cast<float2*>(Ph), *static_cast<const PsArgs*>(a),
                                                   static_cast<hipStream_t>(stream));
    });
}

int ps_second_adjoint_col(int nx, int S, const void* Ph, void* G, const float* mean, const void* a, const void* ad, const void* lin, void* stream) {
    return dispatch_pow2(nx, "spec_ns", [&](auto n) {
        constexpr int N = decltype(n)::value;
        const float2* ph = static_cast<const float2*>(Ph);
        float2* g = static_cast<float2*>(G);
        const PsArgs& args = *static_cast<const PsArgs*>(a);
        const PsAdjSecond& second = *static_cast<const PsAdjSecond*>(ad);
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (lin && S >= 1 && S <= 3) return launch_col_adj<N>(S, ph, g, mean, args, PsAdjSecondLinear{second, static_cast<const float2*>(lin)}, s);
        return launch_col_adj<N>(S, ph, g, mean, args, second, s);
    });
}
#else      // PSPEC_SCALAR_TANGENTS_TU: the launches of K tangents on the scalar system (declared at the head of this file)
int ps_scalar_tangents_col(int nx, int S, const void* Ph, void* G, void* W, void* A, const float* mean, const void* a, int emit, const void* fc,
                           const void* sc, void* stream, const void* st, const void* li, const void* ts, const void* tu) {
    return dispatch_pow2(nx, "spec_ns", [&](auto n) {
        return launch_col_stage<decltype(n)::value>(S, static_cast<const float2*>(Ph), static_cast<float2*>(G), static_cast<float2*>(W),
                                                    static_cast<float2*>(A), mean, *static_cast<const PsArgs*>(a), emit,
                                                    static_cast<const PsForce*>(fc), static_cast<const PsScalar*>(sc),
                                                    static_cast<hipStream_t>(stream), static_cast<const PsStoch*>(st),
                                                    static_cast<const PsLinear*>(li), nullptr, static_cast<const PsTangents*>(ts), nullptr,
                                                    static_cast<const PsTangentsScalar*>(tu));
    });
}

int ps_scalar_tangents_row(int ny, const void* G, void* Ph, const void* a, void* stream, const void* gr, int buoyant, int K) {
    return dispatch_pow2(ny, "spec_ns", [&](auto n) {
        constexpr int N = decltype(n)::value;
        const float2* g = static_cast<const float2*>(G);
        float2* ph = static_cast<float2*>(Ph);
        const PsArgs& args = *static_cast<const PsArgs*>(a);
        hipStream_t s = static_cast<hipStream_t>(stream);
        return buoyant ? launch_row_tans_scalar<N>(g, ph, args, K, s, *static_cast<const PsBuoyGrad*>(gr))
                       : launch_row_tans_scalar<N>(g, ph, args, K, s, *static_cast<const PsGrad*>(gr));
    });
}
#endif
