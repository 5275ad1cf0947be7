/*
 * nns.h -- C ABI of libnns_hip.so, the MI355X (gfx950) residual engine behind the call surface of
 * mhw32/neural-navier-stokes (src/boundary.py, src/chorin_fd, src/direct_fd, src/chorin_spectral,
 * src/neural_spectral).  The reference is pure Python with no FFI of its own:
 * the entry points below are what a ctypes binding on the reference side would bind for each of
 * its operators; every declaration cites the reference symbol (file:line) it replaces.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless the name ends in
 *     _host; buffers are caller-owned and caller-allocated (workspace sizes via the *_workspace
 *     query functions); the library never allocates or frees device memory in a launch function;
 *   - one call = one stream-ordered enqueue on `stream` (a hipStream_t; NULL = default stream),
 *     no host synchronisation unless the function says so;
 *   - fields are C-contiguous [batch, nx, ny]; element [b][i][j] at (b*nx + i)*ny + j;
 *     suffix _f32 / _f64 is the storage type of the fields (arithmetic is done in that type
 *     unless stated);
 *   - return value: 0 on success, a negative nns_status otherwise; never throws, never aborts;
 *     nns_last_error() returns a thread-local message for the last failure;
 *   - boundary lists (nns_bc_list) are small host structs passed by pointer and copied into
 *     kernel arguments.
 */
#ifndef NNS_H
#define NNS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NNS_VERSION_MAJOR 0
#define NNS_VERSION_MINOR 1

typedef enum nns_status {
    NNS_OK = 0,
    NNS_ERR_INVALID_ARG = -1,   /* bad size / null pointer / unsupported combination       */
    NNS_ERR_UNSUPPORTED = -2,   /* valid request this build has no kernel for              */
    NNS_ERR_LAUNCH = -3,        /* HIP reported a launch/runtime error (see last_error)    */
    NNS_ERR_WORKSPACE = -4      /* workspace too small                                     */
} nns_status;

/* ---- boundary conditions: src/boundary.py:1-86 ------------------------------------------- */
enum { NNS_BC_DIRICHLET = 0, NNS_BC_NEUMANN = 1 };                 /* .type,  :32,:54          */
enum { NNS_SIDE_LEFT = 0,   /* A[0, :]   src/boundary.py:39-40 */
       NNS_SIDE_RIGHT = 1,  /* A[-1, :]  :41-42 */
       NNS_SIDE_BOTTOM = 2, /* A[:, 0]   :43-44 */
       NNS_SIDE_TOP = 3 };  /* A[:, -1]  :45-46 */
#define NNS_MAX_BC 8
typedef struct nns_bc_list {
    int32_t n;                       /* number of entries, applied in list order (corners!)   */
    int32_t kind[NNS_MAX_BC];
    int32_t side[NNS_MAX_BC];
    double value[NNS_MAX_BC];
    double dx[NNS_MAX_BC];           /* each BC object carries its own dx, dy (:23)            */
    double dy[NNS_MAX_BC];
} nns_bc_list;

const char* nns_last_error(void);
int nns_version(void);                                  /* major*1000 + minor                  */
/* Fills name (<= cap bytes), CU count, and HBM bytes of the current device. */
int nns_device_info(char* name_host, int cap, int* cu_count_host, size_t* hbm_bytes_host);

/* DirichletBoundaryCondition.apply / NeumannBoundaryCondition.apply (src/boundary.py:34-48,
 * :56-86) for a whole list, in list order, in place, on every grid of the batch. */
int nns_bc_apply_f32(float* A, int batch, int nx, int ny, const nns_bc_list* bcs_host, void* stream);
int nns_bc_apply_f64(double* A, int batch, int nx, int ny, const nns_bc_list* bcs_host, void* stream);

/* ---- chorin_fd: src/chorin_fd/simulate.py ------------------------------------------------ */
/* _explicit_predictor_step (:63-91): AB2 advection (both differences along axis 0 -- reference
 * quirk) + AB2 5-point diffusion on the interior, edges copied from un/vn.  out: ui, vi. */
int nns_fd_predictor_explicit_f32(const float* un, const float* vn, const float* un1, const float* vn1,
                                  float* ui, float* vi, int batch, int nx, int ny,
                                  double dt, double dx, double dy, double nu, void* stream);
int nns_fd_predictor_explicit_f64(const double* un, const double* vn, const double* un1, const double* vn1,
                                  double* ui, double* vi, int batch, int nx, int ny,
                                  double dt, double dx, double dy, double nu, void* stream);

/* _semi_implicit_predictor_step (:93-167): AB2 advection + Crank-Nicolson ADI; the dense
 * np.linalg.solve calls (:137,:153,:159,:165) become constant-coefficient Thomas solves, one
 * thread per column, BOTH along axis 0 as in the reference (needs nx == ny).  work: 4*batch*nx*ny
 * elements of scratch. */
size_t nns_fd_predictor_adi_workspace(int batch, int nx, int ny, int elem_size);
int nns_fd_predictor_adi_f32(const float* un, const float* vn, const float* un1, const float* vn1,
                             float* ui, float* vi, float* work, int batch, int nx, int ny,
                             double dt, double dx, double dy, double nu, void* stream);
int nns_fd_predictor_adi_f64(const double* un, const double* vn, const double* un1, const double* vn1,
                             double* ui, double* vi, double* work, int batch, int nx, int ny,
                             double dt, double dx, double dy, double nu, void* stream);

/* The same predictor on a COLUMN slab [nx][nyl] of a square nx x nx grid (halo / boundary columns 0 and nyl-1 are copied
 * from un like any edge): both solves run along axis 0, so column slabs need no communication for them -- the
 * multi-GPU form of the ADI step (nns/slab.py: SlabChorinFD(method='semi_implicit')).  Identical arithmetic; only
 * the nx == ny check is waived. */
int nns_fd_predictor_adi_colslab_f32(const float* un, const float* vn, const float* un1, const float* vn1,
                                     float* ui, float* vi, float* work, int batch, int nx, int nyl,
                                     double dt, double dx, double dy, double nu, void* stream);
int nns_fd_predictor_adi_colslab_f64(const double* un, const double* vn, const double* un1, const double* vn1,
                                     double* ui, double* vi, double* work, int batch, int nx, int nyl,
                                     double dt, double dx, double dy, double nu, void* stream);

/* dx2dy2C of _get_pressure (:186-188): backward-difference divergence RHS, zero on the edge. */
int nns_fd_pressure_rhs_f32(const float* ui, const float* vi, float* C, int batch, int nx, int ny,
                            double dt, double dx, double dy, double rho, void* stream);
int nns_fd_pressure_rhs_f64(const double* ui, const double* vi, double* C, int batch, int nx, int ny,
                            double dt, double dx, double dy, double rho, void* stream);

/* The SOR loop of _get_pressure (:190-200): in-place lexicographic Gauss-Seidel with
 * over-relaxation, evaluated in anti-diagonal wavefront order (bitwise-identical update order),
 * several sweeps in flight skewed by two fronts.  Stops after the first sweep whose
 * max|p - pPrev| <= tol, or after max_sweeps (= nit-1) sweeps.  p is updated in place.
 * info[2*b] = sweeps done, info[2*b+1] = last err (as the field type), per grid b.
 * Zero-sweep rule: the reference's `while err > tol and it < nit` starts from err = 1, so with
 * tol >= 1 (or a tol that is NaN) or max_sweeps = 0 no sweep runs: info = (0, 1), p untouched.
 * work: nns_fd_sor_workspace() bytes. One workgroup per grid ("replicas only" across GPUs). */
size_t nns_fd_sor_workspace(int batch, int nx, int ny, int elem_size);
/* (The sweeps run speculatively in batches; a stop inside a batch costs a restore + replay.  nns_fd_sor_hint_* take `hint` [batch][2] -- the info of the
 * PREVIOUS solve of the same grids in a time loop, device memory, may be the same buffer as info, NULL = none -- and size the first batch by its sweep
 * count: a scheduling hint only, the results do not depend on it.) */
int nns_fd_sor_f32(float* p, const float* C, float* info, void* work, int batch, int nx, int ny,
                   double dx, double dy, double beta, double tol, int max_sweeps, void* stream);
int nns_fd_sor_f64(double* p, const double* C, double* info, void* work, int batch, int nx, int ny,
                   double dx, double dy, double beta, double tol, int max_sweeps, void* stream);
int nns_fd_sor_hint_f32(float* p, const float* C, float* info, const float* hint, void* work, int batch, int nx, int ny,
                        double dx, double dy, double beta, double tol, int max_sweeps, void* stream);
int nns_fd_sor_hint_f64(double* p, const double* C, double* info, const double* hint, void* work, int batch, int nx, int ny,
                        double dx, double dy, double beta, double tol, int max_sweeps, void* stream);

/* ---- corrected / extended solver options (NOT reference behaviour) ----------------
 * Explicit predictor with the true y-advection  v d/dy  (the reference differences along x twice, :73-76,:82-85);
 * oracle: oracle/chorin_fd.py explicit_predictor_corrected. */
int nns_fd_predictor_explicit_corrected_f32(const float* un, const float* vn, const float* un1, const float* vn1,
                                            float* ui, float* vi, int batch, int nx, int ny,
                                            double dt, double dx, double dy, double nu, void* stream);
int nns_fd_predictor_explicit_corrected_f64(const double* un, const double* vn, const double* un1, const double* vn1,
                                            double* ui, double* vi, int batch, int nx, int ny,
                                            double dt, double dx, double dy, double nu, void* stream);
/* Semi-implicit (ADI) predictor with the second tridiagonal solve along axis 1, as an ADI scheme intends (the reference
 * runs both along axis 0 and therefore needs nx == ny); oracle: semi_implicit_predictor_corrected.  Same workspace as
 * nns_fd_predictor_adi; nx != ny allowed. */
int nns_fd_predictor_adi_corrected_f32(const float* un, const float* vn, const float* un1, const float* vn1,
                                       float* ui, float* vi, float* work, int batch, int nx, int ny,
                                       double dt, double dx, double dy, double nu, void* stream);
int nns_fd_predictor_adi_corrected_f64(const double* un, const double* vn, const double* un1, const double* vn1,
                                       double* ui, double* vi, double* work, int batch, int nx, int ny,
                                       double dt, double dx, double dy, double nu, void* stream);
/* Red-black SOR: the update formula, relaxation factor, stopping rule (max|p - pPrev| <= tol) and sweep cap of
 * nns_fd_sor, with the points of one colour ((i + j) even, then odd) relaxed in parallel: two barriers per sweep
 * instead of nx + ny fronts.  Same info layout.  oracle: get_pressure_redblack (bitwise).
 * Grids whose p and C fit LDS (2 nx ny elements <= 150 KB) are solved by one workgroup each, work may be NULL.
 * Larger grids run every half-sweep as a chip-wide launch: all 2 max_sweeps launches are enqueued at once and turn
 * themselves off on the device once a sweep's error is <= tol (no host round trip); they need
 * nns_fd_sor_redblack_workspace(batch, nx, ny, elem_size, max_sweeps) bytes of device memory in `work` (0 = fits LDS). */
size_t nns_fd_sor_redblack_workspace(int batch, int nx, int ny, int elem_size, int max_sweeps);
int nns_fd_sor_redblack_f32(float* p, const float* C, float* info, void* work, int batch, int nx, int ny,
                            double dx, double dy, double beta, double tol, int max_sweeps, void* stream);
int nns_fd_sor_redblack_f64(double* p, const double* C, double* info, void* work, int batch, int nx, int ny,
                            double dx, double dy, double beta, double tol, int max_sweeps, void* stream);

/* Multigrid solve of the same pressure equation (an option of the build; src/chorin_fd/simulate.py:186-196 is the equation, not the method):
 * on interior points  dy^2 (p[i+1,j] + p[i-1,j] - 2p) + dx^2 (p[i,j+1] + p[i,j-1] - 2p) = C[i,j]  -- the fixed point of the reference's SOR
 * update -- with p's boundary ring as Dirichlet data, read and never written.  C as for nns_fd_sor (nns_fd_pressure_rhs, the reference's dx2dy2C).
 * V(2,2) cycles: red-black Gauss-Seidel smoothing, per-axis coarsening n -> (n - 1) / 2 + 1 by node coordinate (any n >= 5), linear
 * prolongation, restriction = scaled transpose, exact coarsest solve; restatement: tests/mg_oracle.py.  Each grid of the batch stops on its own,
 * on the device, after the cycle in which max|r_k| <= tol max|r_0| or max|r_k| >= 0.9 max|r_(k-1)| (the rounding floor); a grid with
 * max|r_0| = 0 runs no cycle and keeps p bitwise.  info[b] = (cycles done, max|r_k| / max|r_0|) in p's type ((0, 0) for a zero residual).
 * A NaN or infinite max|r_0| (a NaN or Inf in C, in p's interior or in its boundary ring) is never a zero residual: the grid runs no cycle,
 * keeps p bitwise and reports (0, NaN).
 * cycles: at most this many cycles are enqueued by this call, no host synchronisation.  resume = 0 starts a solve (measures max|r_0|);
 * resume = 1 continues the solve whose state `work` holds from an earlier call on the same p, C, info.  The first batch int32 of `work` are
 * the grids' active flags (1 = not stopped), readable by the caller between calls.
 * work: nns_fd_poisson_mg_workspace bytes, written to *bytes.  NNS_ERR_UNSUPPORTED: a grid axis < 5 nodes, a level's cell aspect ratio > 2,
 * a coarsest level of more than 33 nodes on an axis, batch > 65535. */
int nns_fd_poisson_mg_workspace(int batch, int nx, int ny, int elem_size, size_t* bytes);
int nns_fd_poisson_mg_f32(float* p, const float* C, float* info, void* work, int batch, int nx, int ny,
                          double dx, double dy, double tol, int cycles, int resume, void* stream);
int nns_fd_poisson_mg_f64(double* p, const double* C, double* info, void* work, int batch, int nx, int ny,
                          double dx, double dy, double tol, int cycles, int resume, void* stream);

/* One red-black HALF-sweep on a row slab p[nxl][ny] whose rows 0 and nxl-1 are halo / boundary rows (not written);
 * local row i is global row gi0 + i (that fixes the colours).  Multi-workgroup.  *err_bits (4 bytes for f32, 8 for f64,
 * zeroed by the caller) receives max|p_new - p_old| as an IEEE bit pattern via an unsigned atomic max.  Building block
 * of the sharded pressure solve (nns/slab.py: SlabPressure) and of red-black SOR on grids too large for LDS. */
int nns_fd_sor_redblack_halfsweep_f32(float* p, const float* C, void* err_bits, int nxl, int ny, int gi0, int colour,
                                      double dx, double dy, double beta, void* stream);
int nns_fd_sor_redblack_halfsweep_f64(double* p, const double* C, void* err_bits, int nxl, int ny, int gi0, int colour,
                                      double dx, double dy, double beta, void* stream);
/* The same half-sweep as one link of a pre-enqueued chain: it runs only if *prev_err_bits (the previous sweep's error, same
 * bit-pattern format, already max-reduced over the ranks by the caller) is > tol -- the reference's `while err > tol`
 * (src/chorin_fd/simulate.py:190) evaluated on the device; a skipped colour-1 half-sweep stores the all-ones-but-sign (NaN)
 * pattern in *err_bits so that everything after it stays off.  No host round trip per sweep. */
int nns_fd_sor_redblack_halfsweep_gated_f32(float* p, const float* C, void* err_bits, const void* prev_err_bits, double tol,
                                            int nxl, int ny, int gi0, int colour, double dx, double dy, double beta, void* stream);
int nns_fd_sor_redblack_halfsweep_gated_f64(double* p, const double* C, void* err_bits, const void* prev_err_bits, double tol,
                                            int nxl, int ny, int gi0, int colour, double dx, double dy, double beta, void* stream);

/* spatial_coarsen (src/utils.py:13-60): block means over agg_x x agg_y cells of the [nt][nx][ny] sequences u, v, p into
 * [nt][nx/agg_x][ny/agg_y], one launch for the three fields.  The add order of numpy.mean (pairwise) is reproduced, so
 * float64 results are bit-identical to the reference's.  jfill = number of coarse COLUMNS the reference fills per row:
 * its column loop runs to ny // agg_x (:49), cells beyond stay 0; pass ny / agg_y for the plain block mean. */
int nns_coarsen_f32(const float* u, const float* v, const float* p, float* cu, float* cv, float* cp, int nt, int nx, int ny,
                    int agg_x, int agg_y, int jfill, void* stream);
int nns_coarsen_f64(const double* u, const double* v, const double* p, double* cu, double* cv, double* cp, int nt, int nx, int ny,
                    int agg_x, int agg_y, int jfill, void* stream);

/* step (:212-234) of the EXPLICIT method as ONE launch, one workgroup per grid: _explicit_predictor_step, the velocity boundary lists, _get_pressure
 * (right-hand side + the lexicographic SOR solve, tol / max_sweeps as nns_fd_sor_*), the pressure boundary list, _correction_step -- bitwise the
 * sequence nns_fd_predictor_explicit(_corrected) / nns_bc_apply x 2 / nns_fd_pressure_rhs / nns_fd_sor / nns_bc_apply / nns_fd_correction (the same
 * per-point functions).  p is updated in place (as the reference mutates it) and also written to p_copy when that is not NULL (a trajectory slot);
 * u_out, v_out receive the new velocities (they hold the intermediate ones on the way: they must not alias an input field); info [batch][2] =
 * (sweeps, last err; the zero-sweep rule of nns_fd_sor_* holds: with tol >= 1 or max_sweeps = 0 info = (0, 1) and p leaves as the pressure boundary list's
 * image of the p that came in); hint: as nns_fd_sor_hint_* (the previous step's info or NULL); work: nns_fd_sor_workspace(batch, nx, ny, elem) bytes.  Applies when p and its right-hand side fit one workgroup's LDS
 * (nns_fd_step_explicit_fits: 64 x 64 float64, 96 x 96 float32 and below); NNS_ERR_UNSUPPORTED otherwise: use the separate calls. */
int nns_fd_step_explicit_fits(int nx, int ny, int elem_size);
int nns_fd_step_explicit_f32(const float* un, const float* vn, const float* un1, const float* vn1, float* p, const nns_bc_list* u_bc, const nns_bc_list* v_bc,
                             const nns_bc_list* p_bc, float* u_out, float* v_out, float* p_copy, float* info, const float* hint, void* work, int batch, int nx, int ny,
                             double dt, double dx, double dy, double rho, double nu, double beta, double tol, int max_sweeps, int corrected, void* stream);
int nns_fd_step_explicit_f64(const double* un, const double* vn, const double* un1, const double* vn1, double* p, const nns_bc_list* u_bc, const nns_bc_list* v_bc,
                             const nns_bc_list* p_bc, double* u_out, double* v_out, double* p_copy, double* info, const double* hint, void* work, int batch, int nx, int ny,
                             double dt, double dx, double dy, double rho, double nu, double beta, double tol, int max_sweeps, int corrected, void* stream);

/* _correction_step (:204-210): u = u* - dt/(2dx) d0x p, v = v* - dt/(2dy) d0y p; edges from u*. */
int nns_fd_correction_f32(const float* ui, const float* vi, const float* p, float* u, float* v,
                          int batch, int nx, int ny, double dt, double dx, double dy, void* stream);
int nns_fd_correction_f64(const double* ui, const double* vi, const double* p, double* u, double* v,
                          int batch, int nx, int ny, double dt, double dx, double dy, void* stream);

/* ---- direct_fd: src/direct_fd/simulate.py (axis 1 = x there) ------------------------------- */
/* _build_up_b (:56-66). */
int nns_fd_build_b_f32(const float* u, const float* v, float* b, int batch, int nx, int ny,
                       double dt, double dx, double dy, double rho, void* stream);
int nns_fd_build_b_f64(const double* u, const double* v, double* b, int batch, int nx, int ny,
                       double dt, double dx, double dy, double rho, void* stream);
/* _pressure_poisson (:68-88): exactly nit Jacobi sweeps, the p BC list applied after every sweep.
 * p is updated in place; tmp is a scratch field of the same size (ping-pong). */
int nns_fd_jacobi_f32(float* p, float* tmp, const float* b, int batch, int nx, int ny,
                      double dx, double dy, int nit, const nns_bc_list* p_bc_host, void* stream);
int nns_fd_jacobi_f64(double* p, double* tmp, const double* b, int batch, int nx, int ny,
                      double dx, double dy, int nit, const nns_bc_list* p_bc_host, void* stream);
/* The u, v update of step (:98-118): upwind advection, central grad p / (2 rho), 5-point
 * diffusion.  un, vn -> u, v (edges copied); must not alias. */
int nns_fd_direct_update_f32(const float* un, const float* vn, const float* p, float* u, float* v,
                             int batch, int nx, int ny, double dt, double dx, double dy,
                             double rho, double nu, void* stream);
int nns_fd_direct_update_f64(const double* un, const double* vn, const double* p, double* u, double* v,
                             int batch, int nx, int ny, double dt, double dx, double dy,
                             double rho, double nu, void* stream);

/* ---- periodic-box Navier-Stokes residual (north-star operators; no reference symbol, SURVEY.md
 *      section 8 row a17; defined by oracle/periodic.py) --------------------------------------- */
/* r_u = (u-u_prev)/dt + u u_x + v u_y + p_x/rho - nu lap u ; r_v likewise ; r_div = u_x + v_y.
 * FD back-end: central differences, stencil = 5 or 9 (Mehrstellen) point Laplacian. */
int nns_fd_residual_f32(const float* u, const float* v, const float* p, const float* u_prev,
                        const float* v_prev, float* r_u, float* r_v, float* r_div,
                        int batch, int nx, int ny, double dt, double dx, double dy,
                        double rho, double nu, int stencil, void* stream);
int nns_fd_residual_f64(const double* u, const double* v, const double* p, const double* u_prev,
                        const double* v_prev, double* r_u, double* r_v, double* r_div,
                        int batch, int nx, int ny, double dt, double dx, double dy,
                        double rho, double nu, int stencil, void* stream);
/* The FD residual on local rows [row_begin, row_end) of a ROW SLAB [batch][nx_local][ny] (grids sharded by rows over ranks,
 * nns/slab.py): rows -1 and nx_local come from halo_top / halo_bot ([3 (u, v, p)][batch][ny] messages from the ring
 * neighbours).  Interior rows [1, nx_local-1) never touch the halos, so they can be launched while the exchange is in
 * flight and the two edge rows afterwards ("overlap interior compute with halo"). */
int nns_fd_residual_halo_f32(const float* u, const float* v, const float* p, const float* u_prev, const float* v_prev,
                             const float* halo_top, const float* halo_bot, float* r_u, float* r_v, float* r_div,
                             int batch, int nx_local, int ny, int row_begin, int row_end, double dt, double dx, double dy,
                             double rho, double nu, int stencil, void* stream);
int nns_fd_residual_halo_f64(const double* u, const double* v, const double* p, const double* u_prev, const double* v_prev,
                             const double* halo_top, const double* halo_bot, double* r_u, double* r_v, double* r_div,
                             int batch, int nx_local, int ny, int row_begin, int row_end, double dt, double dx, double dy,
                             double rho, double nu, int stencil, void* stream);
/* Vector-Jacobian product of the FD residual (the physics-informed loss' backward;
 * oracle/periodic.py: fd_residual_vjp).  g_* = dLoss/dr_*; outputs dLoss/du, /dv, /dp and, when the pointers are
 * non-null, dLoss/du_prev = -g_u/dt, dLoss/dv_prev = -g_v/dt.  Adjoint stencils (D^T = -D, L^T = L); p does not enter. */
int nns_fd_residual_bwd_f32(const float* u, const float* v, const float* g_u, const float* g_v, const float* g_div,
                            float* grad_u, float* grad_v, float* grad_p, float* grad_u_prev, float* grad_v_prev,
                            int batch, int nx, int ny, double dt, double dx, double dy,
                            double rho, double nu, int stencil, void* stream);
int nns_fd_residual_bwd_f64(const double* u, const double* v, const double* g_u, const double* g_v, const double* g_div,
                            double* grad_u, double* grad_v, double* grad_p, double* grad_u_prev, double* grad_v_prev,
                            int batch, int nx, int ny, double dt, double dx, double dy,
                            double rho, double nu, int stencil, void* stream);
/* Vector-Jacobian product of the spectral residual (oracle/periodic.py: spectral_residual_vjp): two fused passes like
 * the forward (columns, then rows), three packed forward (`precise` as for nns_spec_residual_f32) and three inverse (float32)
 * LDS-resident transforms per line -- the conjugate spectral multiplies.  grad_u_prev / grad_v_prev may be null.  Axis lengths as for
 * nns_spec_residual_f32: powers of two in [64, 1024] on the FFT engine, any other length 3 .. 2048 as circulant matrices in float64. */
int nns_spec_residual_bwd_f32(const float* u, const float* v, const float* g_u, const float* g_v, const float* g_div,
                              float* grad_u, float* grad_v, float* grad_p, float* grad_u_prev, float* grad_v_prev,
                              int batch, int nx, int ny, double dt, double Lx, double Ly, double rho, double nu,
                              int precise, void* stream);
/* Spectral back-end: d/dx <-> i kx, lap <-> -|k|^2 via LDS-resident 1-D FFTs (the operators are
 * separable, so no 2-D transform is materialised): pass 1 transforms columns (axis 0) and leaves
 * the x-part of the residual in r_u, r_v, r_div; pass 2 transforms rows (axis 1) and completes
 * them in place.
 * AXIS LENGTHS.  The FFT engine serves powers of two in [64, 1024] (every BASELINE.json size).  Any other length n in 3 .. 2048 --
 * the reference drivers' own 51 x 51 and 50 x 50 grids (src/chorin_fd/simulate.py:280-281, src/direct_fd/simulate.py:153-154), 96, 2048 --
 * takes, per axis, the same operator as a CIRCULANT matrix applied in float64 (csrc/spectral_dense.hip: O(n) multiply-adds per point,
 * exact to float32 output rounding, `precise` ignored; the first call with a new (n, L) builds the n-vector on the host and copies it,
 * synchronously).  The two axes of one call choose independently (e.g. 96 x 256).  Longer axes fail with NNS_ERR_UNSUPPORTED.
 * `precise` (every nns_spec_residual_* / nns_residual_both_* entry point) selects the arithmetic of the forward transforms:
 *   0  all-float32: the lines are forward-DIFFERENCED in physical space (exact in float32) and the spectral multiply becomes
 *      a bounded filter, so the white rounding noise of a float32 transform is not amplified by k.  First derivatives come
 *      out at float32 accuracy for any input; the viscous term keeps a relative amplification of rms nu pi N / (sqrt(3) L)
 *      per axis (1.9 at 1024^2, nu = 2 pi / 1000: 1.1e-6 rel-L2 against the float64 oracle; <= 4e-6 measured for nu <= 1);
 *   1  the library picks: all-float32 while that factor is <= 8, otherwise as 2.  Entry points that evaluate BOTH directions
 *      (nns_spec_residual_f32, nns_residual_both_f32, nns_spec_residual_bwd_f32) decide once from the larger of the two axes' factors, so
 *      an anisotropic grid never mixes arithmetic; the single-direction entry points (xpass / ypass / rowpass) decide from their own
 *      axis -- callers that combine them (nns/slab.py) resolve the policy themselves and pass 0 or 2.
 *      (API note: until round 1 `precise = 1` meant float64 forward transforms unconditionally; that is `precise = 2` now.)
 *   2  forward transforms and spectral multiply in float64, inverse in float32 (2-4e-7 rel-L2), whatever the viscosity.
 * nns_spec_residual_bwd_f32 follows the same rule (its three packed pairs per line are differenced the same way);
 * nns_spec_derivs_f32: 0 = plain all-float32, non-zero = float64 forward. */
int nns_spec_residual_f32(const float* u, const float* v, const float* p, const float* u_prev,
                          const float* v_prev, float* r_u, float* r_v, float* r_div,
                          int batch, int nx, int ny, double dt, double Lx, double Ly,
                          double rho, double nu, int precise, void* stream);
/* "Stencil + spectral residual on the same inputs" (the unit of BASELINE.json's metric) in two launches instead of three:
 * the spectral column pass, then ONE row pass that completes the spectral residual AND evaluates the FD 5-point residual
 * (the formula of nns_fd_residual_f32; second differences as differences of exact float32 first differences): a row pass holds
 * whole rows of u, v, p in registers, so the stencil's j-1 / j+1 neighbours are lane rotates.  Rows i-1 / i+1: in the all-float32
 * mode every line of a workgroup marches down a chunk of consecutive rows (row above parked in LDS, row below = the next row's
 * prefetch: no second read); in the float64-forward mode they are re-read from L2 / memory.
 * nx, ny powers of two in [64, 1024] run this fused form (ny = 1024: one row per wave, whole-wave DPP rotates; shorter rows share a
 * wave).  Results equal those of the two separate calls to rounding.  With ny outside the FFT engine's sizes the call IS the two
 * separate calls (nns_fd_residual_f32 + nns_spec_residual_f32, see its AXIS LENGTHS note); nx alone outside them only swaps the column pass.
 * The six output fields must not overlap the inputs or each other (rows i-1 / i+1 of the inputs are read while other rows'
 * outputs are being written).
 * Measured 11-24 % faster than the two calls at every size (tools/both_sizes_run.py). */
int nns_residual_both_f32(const float* u, const float* v, const float* p, const float* u_prev, const float* v_prev,
                          float* fd_r_u, float* fd_r_v, float* fd_r_div, float* sp_r_u, float* sp_r_v, float* sp_r_div,
                          int batch, int nx, int ny, double dt, double Lx, double Ly, double rho, double nu,
                          int precise, void* stream);
/* Its second launch alone: sp_r_* must hold the partials of nns_spec_residual_xpass_f32 on entry (the split form, for
 * timing the two launches separately and for callers that place an exchange between them). */
int nns_residual_both_rowpass_f32(const float* u, const float* v, const float* p, const float* u_prev, const float* v_prev,
                                  float* fd_r_u, float* fd_r_v, float* fd_r_div, float* sp_r_u, float* sp_r_v, float* sp_r_div,
                                  int batch, int nx, int ny, double dt, double Lx, double Ly, double rho, double nu,
                                  int precise, void* stream);
/* The row pass on a ROW SLAB [batch][nx_local][ny] of grids sharded by rows over ranks (nns/slab.py):
 * the stencil's row above local row 0 / below local row nx_local-1 is read from halo_top / halo_bot, two
 * [3 (u, v, p)][batch][ny] messages holding the neighbour ranks' edge rows; dx is the grid spacing along x (the slab does not
 * know the global row count); nx_local >= 3, any value.  Same arithmetic per point as nns_residual_both_rowpass_f32.
 * halo_field_stride: elements between the u, v and p blocks of a halo message; 0 = batch * ny (a message made for exactly these grids).
 * A larger value lets a call on a CHUNK of the batch read its rows out of a message exchanged once for the whole batch
 * (halo_top + first_grid * ny, stride = whole_batch * ny): nns/slab.py pipelines batch chunks and sends one halo message per step. */
int nns_residual_both_rowpass_halo_f32(const float* u, const float* v, const float* p, const float* u_prev, const float* v_prev,
                                       const float* halo_top, const float* halo_bot,
                                       float* fd_r_u, float* fd_r_v, float* fd_r_div, float* sp_r_u, float* sp_r_v, float* sp_r_div,
                                       int batch, int nx_local, int ny, long halo_field_stride, double dt, double dx, double Ly, double rho, double nu,
                                       int precise, void* stream);
/* The two halves of nns_spec_residual_f32, exposed for slab-decomposed (multi-GPU) use:
 * x-pass on a column slab [nx, ny_local] (needs complete columns), y-pass on a row slab
 * [nx_local, ny] (needs complete rows) which reads the x-parts from r_* and finishes them. */
int nns_spec_residual_xpass_f32(const float* u, const float* v, const float* p,
                                float* r_u, float* r_v, float* r_div, int batch, int nx, int ny,
                                double Lx, double rho, double nu, int precise, void* stream);
/* The column pass on a COLUMN SLAB whose rows arrive from an all-to-all in blocks of seg_rows rows per source rank:
 * u, v, p (and the partials written to r_*) are laid out [src][...][batch][seg_rows][ny] -- row r of grid b of a field
 * starts at field + (r / seg_rows) * seg_stride + b * seg_rows * ny + (r % seg_rows) * ny.  seg_rows: a power of two <= nx.
 * Reading the receive buffer and writing the send buffer of the return all-to-all in place removes the permuting copies on
 * both sides of the column pass.  Same arithmetic per column as nns_spec_residual_xpass_f32. */
int nns_spec_residual_xpass_seg_f32(const float* u, const float* v, const float* p, float* r_u, float* r_v, float* r_div,
                                    int batch, int nx, int ny, int seg_rows, long seg_stride, double Lx, double rho, double nu,
                                    int precise, void* stream);
int nns_spec_residual_ypass_f32(const float* u, const float* v, const float* p, const float* u_prev,
                                const float* v_prev, float* r_u, float* r_v, float* r_div,
                                int batch, int nx, int ny, double dt, double Ly,
                                double rho, double nu, int precise, void* stream);
/* The row passes on a ROW SLAB whose column-pass partials are read where the return all-to-all delivered them (round 4; no copy kernel
 * between the collective and the row pass): part_u / part_v / part_div point at source rank 0's block of each partial field in a buffer laid
 * out [src][field][batch][nx_local][seg_cols], seg_cols = ny / P; element (grid b, row i, column j) of a field sits at
 * part + (j / seg_cols) * seg_stride + (b * nx_local + i) * seg_cols + j % seg_cols -- a row is P contiguous pieces of seg_cols floats.
 * seg_cols: a power of two in [ny / 16, ny] (P <= 16: a register slot of a line never straddles two pieces); seg_stride >= batch * nx_local *
 * seg_cols (3 x that for the [src][3 fields] buffer of nns/slab.py).  r_* / sp_r_*: row slabs [batch][nx_local][ny], written only.
 * Same arithmetic per point as nns_spec_residual_ypass_f32 / nns_residual_both_rowpass_halo_f32 (bitwise the single-process result);
 * ny: a power of two in [64, 1024] (the segmented layout exists for the FFT engine only).
 * No reference counterpart: the reference runs on one device (src/neural_spectral/spectral_ode.py:155-156,165). */
int nns_spec_residual_ypass_seg_f32(const float* u, const float* v, const float* p, const float* u_prev, const float* v_prev,
                                    const float* part_u, const float* part_v, const float* part_div, int seg_cols, long seg_stride,
                                    float* r_u, float* r_v, float* r_div, int batch, int nx, int ny, double dt, double Ly,
                                    double rho, double nu, int precise, void* stream);
int nns_residual_both_rowpass_halo_seg_f32(const float* u, const float* v, const float* p, const float* u_prev, const float* v_prev,
                                           const float* halo_top, const float* halo_bot,
                                           const float* part_u, const float* part_v, const float* part_div, int seg_cols, long seg_stride,
                                           float* fd_r_u, float* fd_r_v, float* fd_r_div, float* sp_r_u, float* sp_r_v, float* sp_r_div,
                                           int batch, int nx_local, int ny, long halo_field_stride, double dt, double dx, double Ly,
                                           double rho, double nu, int precise, void* stream);
/* The arithmetic a `precise` request resolves to for a WHOLE evaluation: 0 (all-float32 transforms on differenced lines) or 2 (float64
 * forward transforms), from both transformed axes and the NNS_SPEC_F64 override -- the one policy implementation, for hosts that call the
 * passes one by one (nns/slab.py). */
int nns_spec_resolve_precise(int precise, double nu, int nx, double Lx, int ny, double Ly);
/* Axis lengths outside the FFT engine's sizes run on circulant matrices (AXIS LENGTHS note above) whose table of (n, L) is built on the host,
 * allocated and copied SYNCHRONOUSLY at the first call that needs it, once per device -- not possible while a stream is being captured into a HIP
 * graph (such a call returns NNS_ERR_UNSUPPORTED).  This builds the table of one axis ahead of time on the current device. */
int nns_spec_dense_warmup(int n, double L);
/* Spectral derivatives of ONE real field (d/dx <-> i kx with the Nyquist mode dropped, lap <-> -|k|^2; definition
 * oracle/periodic.py: spectral_derivs): any of f_x, f_y, f_lap may be NULL.  precise as above. */
int nns_spec_derivs_f32(const float* f, float* f_x, float* f_y, float* f_lap, int batch, int nx, int ny,
                        double Lx, double Ly, int precise, void* stream);
/* 2-D real FFT pair with numpy.fft.rfft2 / irfft2 layout and normalisation (float32 transforms): spec is interleaved
 * complex64 [batch, nx, ny/2+1].  irfft2 uses spec as scratch for its column pass (spec is overwritten). */
int nns_spec_rfft2_f32(const float* f, float* spec, int batch, int nx, int ny, void* stream);
int nns_spec_irfft2_f32(float* spec, float* f, int batch, int nx, int ny, void* stream);

/* ---- pseudo-spectral Navier-Stokes solver on the periodic box [0, Lx) x [0, Ly) (csrc/pspec_kernels.hip; restatement: tests/pspec_oracle.py) --
 * Vorticity-streamfunction form, float32, fields [batch][nx][ny] (axis 0 = x), nx and ny each a power of two in [64, 1024].
 * kx = 2 pi m_x / Lx, ky = 2 pi m_y / Ly (m = the fftfreq index); 2/3-rule mask M = 1 where 3|m_x| < nx and 3|m_y| < ny.
 * State: what = the vorticity spectrum w^ (numpy.fft.rfft2 convention, M w^ = w^, w^(0,0) = 0), COMPACTED to the kept y-wavenumbers
 * j < my1 = (ny - 1) / 3 + 1 and transposed: interleaved complex64 [batch][my1][nx], element [b][j][i] = w^[b][i][j] (i in fftfreq order);
 * mean = the conserved mean velocity (U0, V0), float32 [batch][2].  u = U0 + irfft2(i ky psi^), v = V0 - irfft2(i kx psi^), psi^ = w^ / |k|^2.
 * work: nns_spec_ns_workspace bytes (one workspace serves init, step, step_forced and fields; none of them keeps data in it between calls).
 * Errors: NNS_ERR_INVALID_ARG for a NULL pointer, batch < 1, non-positive or non-finite Lx, Ly, dt, negative nu, nsteps < 0;
 * NNS_ERR_UNSUPPORTED for an axis that is not a power of two in [64, 1024]; NNS_ERR_WORKSPACE for work_bytes below the size query. */
int nns_spec_ns_workspace(int batch, int nx, int ny, size_t* bytes);
/* what = M (i kx v^ - i ky u^), mean = grid means of u, v: projects (u, v) onto divergence-free, band-limited fields. */
int nns_spec_ns_init_f32(const float* u, const float* v, float* what, float* mean, void* work, size_t work_bytes, int batch, int nx, int ny,
                         double Lx, double Ly, void* stream);
/* nsteps steps (0: nothing) of integrating-factor (Lawson) RK4, L = -nu |k|^2, on what in place; N(w^) = -M rfft2(u w_x + v w_y).
 * 8 launches per step plus one per call, no allocation and no host synchronisation (capturable in a HIP graph). */
int nns_spec_ns_step_f32(float* what, const float* mean, void* work, size_t work_bytes, int batch, int nx, int ny, double Lx, double Ly,
                         double dt, double nu, int nsteps, void* stream);
/* u, v [batch][nx][ny] as above and p = irfft2(-M rfft2(2 rho (u_x v_y - u_y v_x)) / |k|^2), p^(0,0) = 0 (derivatives from psi^). */
int nns_spec_ns_fields_f32(const float* what, const float* mean, float* u, float* v, float* p, void* work, size_t work_bytes, int batch,
                           int nx, int ny, double Lx, double Ly, double rho, void* stream);
/* The step with a body force constant in time and a linear drag (restatement: tests/pspec_forced_oracle.py):
 *     w_t + u w_x + v w_y = nu lap w - drag w + g,      g^ = M (i kx f_y^ - i ky f_x^)
 * i.e. u_t + (u . grad) u = -grad p / rho + nu lap u - drag (u - <u>) + f_s with f_s the solenoidal, zero-mean, band-limited part of f; the
 * mean velocity stays conserved and undamped.  Same Lawson RK4 with L = -(nu |k|^2 + drag) and N(w^) = -M rfft2(u w_x + v w_y) + g^ (the
 * same g^ in all four stages).  ghat = g^ in the layout of what, float32 [gbatch][my1][nx][2]: it is what nns_spec_ns_init_f32(f_x, f_y, ...)
 * writes to what.  gbatch = 1: one force shared by every grid; gbatch = batch: one per grid; ghat == NULL requires gbatch == 0 (no force).
 * NNS_ERR_INVALID_ARG for any other gbatch and for a negative or non-finite drag; otherwise the errors, the workspace and the launch
 * count (8 per step plus one per call, no allocation, no host synchronisation, capturable) of nns_spec_ns_step_f32, and with ghat == NULL,
 * gbatch == 0, drag == 0 its result bitwise (the same kernels). */
int nns_spec_ns_step_forced_f32(float* what, const float* mean, const float* ghat, int gbatch, void* work, size_t work_bytes, int batch,
                                int nx, int ny, double Lx, double Ly, double dt, double nu, double drag, int nsteps, void* stream);
/* out [batch][3] float64 (device) = per grid, from what (and ghat, gbatch as above) by Parseval over the stored half spectrum:
 *     E = 1/2 <|u - <u>|^2> = 1/2 sum wt |w^|^2 / |k|^2    (fluctuation energy; the total is E + (U0^2 + V0^2) / 2)
 *     Z = 1/2 <w^2>         = 1/2 sum wt |w^|^2
 *     P = <f_s . u>         =     sum wt Re(psi^ conj g^)   (0 without a force)
 * wt = 1 on the j = 0 line and 2 on j > 0, all normalised by (nx ny)^2, so that dE/dt = P - 2 nu Z - 2 drag E.  float64 sums in a fixed
 * order (no atomics): they repeat bitwise and a grid's numbers do not depend on its batch neighbours.  No workspace; one launch. */
int nns_spec_ns_diag_f32(const float* what, const float* ghat, int gbatch, double* out, int batch, int nx, int ny, double Lx, double Ly,
                         void* stream);
/* A passive scalar theta (temperature, dye), one per grid, advected by the flow and not acting on it (restatement:
 * tests/pspec_scalar_oracle.py).  The total field is G . x + theta with a uniform mean gradient G = (gx, gy); theta is its periodic part:
 *     theta_t + u theta_x + v theta_y = kappa lap theta - (gx u + gy v)
 * State: that = M_theta rfft2(theta) in the layout of what, float32 [batch][my1][nx][2], where M_theta is the 2/3 mask with the (0, 0) mode
 * KEPT (the mean of theta is part of the state).  (w^, theta^) is one system under the same Lawson RK4: L_theta = -kappa |k|^2 (the drag does
 * not act on the scalar), N_theta = -M_theta rfft2(u (theta_x + gx) + v (theta_y + gy)) with every stage's own velocity, means included, so
 * that d<theta>/dt = -G . (U0, V0) and d/dt 1/2 <theta'^2> = -G . <u theta'> - kappa <|grad theta|^2>.  w^ evolves bitwise as without the scalar.
 * The scalar calls take a workspace of nns_spec_ns_scalar_workspace bytes (>= nns_spec_ns_workspace; it serves every nns_spec_ns_* call). */
int nns_spec_ns_scalar_workspace(int batch, int nx, int ny, size_t* bytes);
/* that = M_theta rfft2(theta), theta float32 [batch][nx][ny]: keeps the band-limited part of theta, its mean included. */
int nns_spec_ns_scalar_init_f32(const float* theta, float* that, void* work, size_t work_bytes, int batch, int nx, int ny, void* stream);
/* theta [batch][nx][ny] = irfft2 of the state. */
int nns_spec_ns_scalar_field_f32(const float* that, float* theta, void* work, size_t work_bytes, int batch, int nx, int ny, void* stream);
/* nsteps steps of (what, that) in place.  ghat, gbatch, drag as in nns_spec_ns_step_forced_f32 (ghat == NULL, gbatch == 0, drag == 0: the
 * unforced flow); kappa >= 0 and finite, gx and gy finite, else NNS_ERR_INVALID_ARG; NNS_ERR_WORKSPACE for work_bytes below
 * nns_spec_ns_scalar_workspace; otherwise the errors of nns_spec_ns_step_forced_f32.  The scalar rides in the flow's launches: 8 per step
 * plus one per call, no allocation, no host synchronisation (capturable). */
int nns_spec_ns_step_scalar_f32(float* what, float* that, const float* mean, const float* ghat, int gbatch, void* work, size_t work_bytes,
                                int batch, int nx, int ny, double Lx, double Ly, double dt, double nu, double drag, double kappa, double gx,
                                double gy, int nsteps, void* stream);
/* out [batch][4] float64 (device) = per grid, by Parseval over the stored half spectrum without its (0, 0) mode (wt and normalisation of
 * nns_spec_ns_diag_f32; u^ = i ky psi^, v^ = -i kx psi^ from what):
 *     variance    = 1/2 <theta'^2>            = 1/2 sum wt |theta^|^2
 *     dissipation = kappa <|grad theta|^2>    = kappa sum wt |k|^2 |theta^|^2
 *     flux_x      = <u theta'>                = sum wt Re(u^ conj theta^),      flux_y = <v theta'> likewise
 * so that d variance / dt = -(gx flux_x + gy flux_y) - dissipation.  float64 sums in a fixed order (no atomics); no workspace; one launch. */
int nns_spec_ns_scalar_diag_f32(const float* what, const float* that, double* out, int batch, int nx, int ny, double Lx, double Ly,
                                double kappa, void* stream);
/* Shell spectra and spectral transfers (restatement: tests/pspec_spectrum_oracle.py).  Shells of width dk = min(2 pi / Lx, 2 pi / Ly) centred
 * on k_s = s dk: the stored mode (m_x, j) belongs to shell s = floor(|k| / dk + 1/2), in float64; nshell = the shell of the band's corner
 * (|m_x| = (nx - 1) / 3, j = my1 - 1) + 1, so an elongated box has many shells.  Shell 0 holds the (0, 0) mode alone, which contributes
 * nothing.  Every per-shell number is the sum over the shell's stored modes of wt (...) / (nx ny)^2, wt as in nns_spec_ns_diag_f32.
 * nns_spec_ns_shells: host only.  NNS_ERR_INVALID_ARG for a NULL pointer or a bad Lx, Ly; NNS_ERR_UNSUPPORTED for the axes. */
int nns_spec_ns_shells(int nx, int ny, double Lx, double Ly, int* nshell, double* dk);
/* out [batch][4][nshell] float64 (device) = per grid and shell, from what, that (NULL: no scalar) and ghat, gbatch as in nns_spec_ns_diag_f32:
 *     E = 1/2 sum wt |w^|^2 / |k|^2,   Z = 1/2 sum wt |w^|^2,   F = sum wt Re(psi^ conj g^),   V = 1/2 sum wt |theta^|^2 (k != 0)
 * whose sums over the shells are the E, Z, P of nns_spec_ns_diag_f32 and the variance of nns_spec_ns_scalar_diag_f32; a row without its source
 * (F without ghat, V without that) is zeros.  One launch, one wave per (grid, shell), float64 sums in a fixed order (no atomics): a grid's
 * numbers repeat bitwise and depend neither on the batch nor on the grid's place in it.  No workspace, no allocation, no host
 * synchronisation (capturable).  NNS_ERR_INVALID_ARG for a NULL what or out, batch < 1, a bad gbatch, Lx, Ly, or an nshell that is not
 * nns_spec_ns_shells'; NNS_ERR_UNSUPPORTED for the axes. */
int nns_spec_ns_spectrum_f32(const float* what, const float* that, const float* ghat, int gbatch, double* out, int nshell, int batch, int nx,
                             int ny, double Lx, double Ly, void* stream);
/* out [batch][3][nshell] float64 (device) = the nonlinear transfers into every shell, from ONE evaluation of the step's dealiased nonlinear
 * term in the co-moving frame (U0 = V0 = 0: a uniform flow transfers nothing) and, for the scalar, without the mean gradient:
 *     T_E = sum wt Re(conj w^ N^) / |k|^2,   T_Z = sum wt Re(conj w^ N^),   T_theta = sum wt Re(conj theta^ N_theta^) (k != 0; zeros with that == NULL)
 * N^ = -M rfft2(u w_x + v w_y), N_theta^ = -M_theta rfft2(u theta_x + v theta_y); each sums to 0 over the shells, to float32 rounding, and
 * dE(s)/dt = T_E(s) + F(s) - 2 nu Z(s) - 2 drag E(s).  Four launches plus one that zeroes a corner of work: the step's stage-0 column pass
 * and row pass, a column pass that forms the per-mode products, and the shell sums of nns_spec_ns_spectrum_f32 (same determinism).  what and
 * that are only read.  work: nns_spec_ns_workspace bytes, nns_spec_ns_scalar_workspace with that; no allocation, no host synchronisation
 * (capturable).  Errors as nns_spec_ns_spectrum_f32, plus NULL work and NNS_ERR_WORKSPACE for work_bytes below the size query. */
int nns_spec_ns_transfer_f32(const float* what, const float* that, double* out, int nshell, void* work, size_t work_bytes, int batch, int nx,
                             int ny, double Lx, double Ly, void* stream);
/* Boussinesq buoyancy (restatement: tests/pspec_buoyant_oracle.py): the scalar acts on the flow through b theta', b = (bx, by) uniform and
 * theta' = theta - <theta>:
 *     u_t + (u . grad) u = -grad p / rho + nu lap u - drag (u - <u>) + f_s + b theta'
 *     w_t + u w_x + v w_y = nu lap w - drag w + g + (by theta_x - bx theta_y)
 * Only the periodic fluctuation is buoyant: b <theta> would only accelerate the frame and the background G . x is taken as hydrostatic (its
 * curl, a constant, cannot exist on a periodic box), so both are dropped.  (w^, theta^) is one system under the same Lawson RK4 with the term
 * explicit, N_w = -M rfft2(u w_x + v w_y) + g^ + M (i kx by - i ky bx) theta^ with every stage's own theta^; L_w, L_theta and N_theta are those
 * of nns_spec_ns_step_scalar_f32.  The term rides in the row pass: still 8 launches per step plus one per call, no allocation, no host
 * synchronisation (capturable).  bx == by == 0 makes exactly the calls of nns_spec_ns_step_scalar_f32.  NNS_ERR_INVALID_ARG for that == NULL
 * or a non-finite bx, by; otherwise the errors of nns_spec_ns_step_scalar_f32. */
int nns_spec_ns_step_buoyant_f32(float* what, float* that, const float* mean, const float* ghat, int gbatch, void* work, size_t work_bytes,
                                 int batch, int nx, int ny, double Lx, double Ly, double dt, double nu, double drag, double kappa, double gx,
                                 double gy, double bx, double by, int nsteps, void* stream);
/* White-in-time stochastic forcing (restatement: tests/pspec_stochastic_oracle.py): nns_spec_ns_step_buoyant_f32's step -- drag, steady force,
 * scalar and buoyancy, whichever are active; that == NULL: no scalar, and kappa, gx, gy, bx, by are ignored -- and after every complete step n
 *     w^_k  <-  w^_k + sqrt(dt) amp_k xi_k(n, ids[b])        on the kept modes k != (0, 0) (entries of amp elsewhere are ignored)
 * amp: non-negative float32 [my1][nx] (device), the layout of one grid of what, shared by the batch.  xi: a complex standard normal,
 * E |xi|^2 = 1, independent over stored modes, steps and ids, from Philox4x32-10 with key (seed low word, seed high word) and counter
 * (n low, n high, j nx + i, ids[b]); of the outputs x0, x1 are used: u1 = ((x0 >> 8) + 1) 2^-24, u2 = (x1 >> 8) 2^-24,
 * xi = sqrt(-ln u1) (cos 2 pi u2, sin 2 pi u2).  On the j = 0 line the element of -m_x takes the counter of |m_x| and is conjugated, so the
 * line stays Hermitian.  The mean energy input is exact and independent of the state: 1/2 sum wt amp_k^2 / (|k|^2 (nx ny)^2), wt as in
 * nns_spec_ns_diag_f32.  The scalar gets no noise.  clock: int64 [1] (device), the stochastic steps this state has taken, n of the next step;
 * the step advances it on the device (stage 1's column launch; stage 4's evaluates the generator in registers where amp_k != 0), so the call
 * is capturable and a replayed step continues the sequence: still 8 launches per step plus one per call, no allocation, no host
 * synchronisation.  ids: int32 [batch] (device): grids with equal ids get equal noise.  nsteps calls of one step, one call of nsteps steps
 * and graph replays give the same bits.  NNS_ERR_INVALID_ARG for NULL amp, clock or ids; otherwise the errors of
 * nns_spec_ns_step_buoyant_f32 (nns_spec_ns_step_forced_f32 with that == NULL; work: nns_spec_ns_workspace bytes then). */
int nns_spec_ns_step_stochastic_f32(float* what, float* that, const float* mean, const float* ghat, int gbatch, void* work, size_t work_bytes,
                                    int batch, int nx, int ny, double Lx, double Ly, double dt, double nu, double drag, double kappa,
                                    double gx, double gy, double bx, double by, const float* amp, unsigned long long seed, long long* clock,
                                    const int* ids, int nsteps, void* stream);
/* u, v as nns_spec_ns_fields_f32 and the pressure of the buoyant flow: lap p = rho (2 (u_x v_y - u_y v_x) + b . grad theta), that is
 * p^ = p^ of nns_spec_ns_fields_f32 - rho i (k . b) theta^ / |k|^2 on the kept modes, zero mean.  work: nns_spec_ns_scalar_workspace bytes.
 * Errors as nns_spec_ns_fields_f32, plus that == NULL and a non-finite bx, by. */
int nns_spec_ns_fields_buoyant_f32(const float* what, const float* that, const float* mean, float* u, float* v, float* p, void* work,
                                   size_t work_bytes, int batch, int nx, int ny, double Lx, double Ly, double rho, double bx, double by,
                                   void* stream);
/* out [batch][nshell] float64 (device) = the buoyancy production per shell, B(s) = sum wt Re(conj(bx u^ + by v^) theta^) / (nx ny)^2 with
 * u^ = i ky psi^, v^ = -i kx psi^; its sum over the shells is bx flux_x + by flux_y of nns_spec_ns_scalar_diag_f32 and
 * dE(s)/dt = T_E(s) + F(s) - 2 nu Z(s) - 2 drag E(s) + B(s).  One launch, the shells, order of summation and determinism of
 * nns_spec_ns_spectrum_f32; its errors, plus that == NULL and a non-finite bx, by. */
int nns_spec_ns_buoyancy_spectrum_f32(const float* what, const float* that, double* out, int nshell, int batch, int nx, int ny, double Lx,
                                      double Ly, double bx, double by, void* stream);
/* General diagonal linear operator (restatement: tests/pspec_linear_oracle.py): hyperviscosity, hypofriction and the beta effect,
 *     w_t + u w_x + v w_y + beta v' = nu lap w - nu_h (-lap)^p w - drag w - mu (-lap)^-q w + g + (buoyancy) + (noise)       (v' = v - <v>),
 * i.e. per mode lambda_k = -(nu |k|^2 + drag + nu_h |k|^2p + mu |k|^-2q) + i beta kx / |k|^2, lambda_(0,0) = 0, integrated exactly by the
 * Lawson RK4 of the other step entries with the complex factors E = exp(lambda dt / 2), E^2 = exp(lambda dt): the step of
 * nns_spec_ns_step_stochastic_f32 (force, scalar, buoyancy and noise, whichever are active) with that operator on the vorticity.
 * lin: float32 [my1][nx][2] (device) = (Re, Im)(lambda_k dt / 2), the layout of one grid of what, shared by the batch; entries off the
 * kept modes and at (0, 0) are ignored.  nu and drag are not arguments: the table holds them.  Re <= 0 is expected, not checked; Im may be
 * given modulo 2 pi.  that == NULL: no scalar, and kappa, gx, gy, bx, by are ignored (the scalar's operator stays -kappa |k|^2).  amp, clock
 * and ids: all NULL (no noise; seed is ignored) or all non-NULL (the kick of nns_spec_ns_step_stochastic_f32 after every complete step).
 * Still 8 launches per step plus one per call, no allocation, no host synchronisation: capturable.  NNS_ERR_INVALID_ARG for a NULL lin and
 * for a partial (amp, clock, ids); otherwise the errors and the workspace of nns_spec_ns_step_stochastic_f32. */
int nns_spec_ns_step_linear_f32(float* what, float* that, const float* mean, const float* ghat, int gbatch, void* work, size_t work_bytes,
                                int batch, int nx, int ny, double Lx, double Ly, double dt, double kappa, double gx, double gy, double bx,
                                double by, const float* lin, const float* amp, unsigned long long seed, long long* clock, const int* ids,
                                int nsteps, void* stream);
/* out [batch][2][nshell] float64 (device) = the linear term's rates per shell: D_E(s) = sum wt rate_k |w^_k|^2 / |k|^2 / (nx ny)^2 and D_Z(s)
 * the same without 1 / |k|^2, rate = Re(lambda_k) float64 [my1][nx] (device; the layout of one grid of what, shared by the batch), so that
 * dE/dt|linear = sum_s D_E(s) and dZ/dt|linear = sum_s D_Z(s); with rate = -(nu |k|^2 + drag) they are -2 nu Z(s) - 2 drag E(s).  One launch,
 * the shells, order of summation and determinism of nns_spec_ns_spectrum_f32; its errors, plus rate == NULL. */
int nns_spec_ns_linear_spectrum_f32(const float* what, const double* rate, double* out, int nshell, int batch, int nx, int ny, double Lx,
                                    double Ly, void* stream);
/* Reverse mode of nns_spec_ns_step_forced_f32 (restatement: tests/pspec_adjoint_oracle.py): the vector-Jacobian product of nsteps steps, as
 * fused kernels in the layout of what.  Cotangents are real band-limited fields paired by the plain grid sum <a, b> = sum a b and stored as
 * their spectra (rfft2 convention, unnormalised, the layout of what): no half-spectrum weights.  With N'(s)^T kappa = M [u kappa_x + v kappa_y]
 * - M [kappa_x w_y - kappa_y w_x]^ / |k|^2 (u, v, w_x, w_y of the stage state s), E = exp(-(nu |k|^2 + drag) dt / 2) and lam the cotangent of a
 * step's result, one step backwards is
 *     k4 = dt/6 lam                   r = N'(s3)^T k4    wbar  = E^2 lam + E^2 r
 *     k3 = dt/3 E lam + dt E r        r = N'(s2)^T k3    wbar += E r
 *     k2 = dt/3 E lam + dt/2 r        r = N'(s1)^T k2    wbar += E r
 *     k1 = dt/6 E^2 lam + dt/2 E r    r = N'(s0)^T k1    wbar += r              gbar += k1 + k2 + k3 + k4
 * what0: float32 [nsteps][batch][my1][nx][2], the spectrum at the START of every step (only read); the stage states s1, s2, s3 are recomputed
 * from it by the forward's own kernels, bitwise the forward's.  mean, ghat, gbatch, dt, nu, drag: those of the forward call (the mean flow and
 * g enter as constants; the mean is not differentiated).  lam: float32 [batch][my1][nx][2], in the cotangent of the state after the last step
 * (its part outside the 2/3 band and its (0, 0) mode are ignored), out the cotangent of the state before the first.  gbar: float32
 * [batch][my1][nx][2] or NULL, out the cotangent of g^, ALWAYS one per grid and summed over the steps of the call (a force shared by the batch:
 * sum it over the batch); overwritten, not added to.  Results are zero outside the band and at (0, 0).  A grid's result does not depend on
 * its batch neighbours, and nsteps steps in one call are bitwise nsteps calls of one step, last first.  work: nns_spec_ns_adjoint_workspace
 * bytes (13 compacted fields: it also serves every unscalared nns_spec_ns_* call).  16 launches per step (7 recompute, 9 adjoint), no
 * allocation, no host synchronisation (capturable).  Errors as nns_spec_ns_step_forced_f32. */
int nns_spec_ns_adjoint_workspace(int batch, int nx, int ny, size_t* bytes);
int nns_spec_ns_step_adjoint_f32(const float* what0, const float* mean, const float* ghat, int gbatch, float* lam, float* gbar, void* work,
                                 size_t work_bytes, int batch, int nx, int ny, double Lx, double Ly, double dt, double nu, double drag,
                                 int nsteps, void* stream);
/* Reverse mode of nns_spec_ns_step_scalar_f32 and nns_spec_ns_step_buoyant_f32 (restatement: tests/pspec_scalar_adjoint_oracle.py): the
 * vector-Jacobian product of nsteps steps of the system (w^, theta^), the scalar riding in the launches of nns_spec_ns_step_adjoint_f32.  With
 * (kappa, m) the cotangents of a stage's (N_w, N_theta) and u, v, w, theta of that stage's state,
 *   r_w     = M [u kappa_x + v kappa_y]^ - M [kappa_x w_y - kappa_y w_x + m_x (theta_y + Gy) - m_y (theta_x + Gx)]^ / |k|^2
 *   r_theta = M_theta [u m_x + v m_y - by kappa_x + bx kappa_y]^                       (M_theta keeps the (0, 0) mode)
 * and the Lawson recurrences of nns_spec_ns_step_adjoint_f32 run twice: with E = exp(-(nu |k|^2 + drag) dt / 2) on (lam, kappa, r_w) and with
 * E_theta = exp(-kappa |k|^2 dt / 2), no drag, on (mu, m, r_theta).  what0, that0: [nsteps][batch][my1][nx][2], the spectra at the START of
 * every step (only read; a step's stages are recomputed from them by the forward's own kernels).  lam, mu: [batch][my1][nx][2], in the
 * cotangents of (w^, theta^) after the last step, out those of the pair before the first.  gbar as in nns_spec_ns_step_adjoint_f32 (the
 * vorticity source; the scalar has none); mean, ghat, gbatch, dt, nu, drag, kappa, (gx, gy), (bx, by): the forward's, constants that are not
 * differentiated.  b = (0, 0) is the passive scalar's adjoint.  A grid's result does not depend on its batch neighbours, and nsteps steps in
 * one call are bitwise nsteps calls of one step, last first.  work: nns_spec_ns_scalar_adjoint_workspace bytes (21 compacted fields: it also
 * serves every other nns_spec_ns_* call).  16 launches per step (7 recompute, 9 adjoint), no allocation, no host synchronisation
 * (capturable).  Errors as nns_spec_ns_step_buoyant_f32. */
int nns_spec_ns_scalar_adjoint_workspace(int batch, int nx, int ny, size_t* bytes);
int nns_spec_ns_step_scalar_adjoint_f32(const float* what0, const float* that0, const float* mean, const float* ghat, int gbatch, float* lam,
                                        float* mu, float* gbar, void* work, size_t work_bytes, int batch, int nx, int ny, double Lx, double Ly,
                                        double dt, double nu, double drag, double kappa, double gx, double gy, double bx, double by, int nsteps,
                                        void* stream);
/* Reverse mode of nns_spec_ns_step_linear_f32, with or without its scalar, buoyancy and noise (restatement:
 * tests/pspec_linear_adjoint_oracle.py).  The Lawson factor E_k = exp(lambda_k dt / 2) is complex with E(-k) = conj(E(k)); under the grid
 * sum's pairing of real fields its transpose is multiplication by conj(E_k), so the recurrences of nns_spec_ns_step_adjoint_f32 (and, for the
 * scalar, of nns_spec_ns_step_scalar_adjoint_f32 with the real E_theta) hold with conj(E), conj(E^2) read from the forward's table lin.  The
 * white-in-time kick of a stochastic step is added after the step and does not depend on the state: its Jacobian is the identity and the
 * saved start spectra carry it, so the adjoint of a stochastic step is this call (or, without a table, the two above) on the spectra the
 * noisy forward saved; the generator is never run.  that0 == NULL and mu == NULL: no scalar (kappa, gx, gy, bx, by are ignored; work:
 * nns_spec_ns_adjoint_workspace bytes); both non-NULL: the scalar's, buoyant with b != 0 (work: nns_spec_ns_scalar_adjoint_workspace bytes).
 * nu and drag are not arguments: the table holds them.  Every other argument as in those two calls; 16 launches per step (7 recompute, 9
 * adjoint), no allocation, no host synchronisation (capturable).  NNS_ERR_INVALID_ARG for a NULL lin and when exactly one of that0, mu is
 * NULL; otherwise the errors of nns_spec_ns_step_adjoint_f32 / nns_spec_ns_step_scalar_adjoint_f32. */
int nns_spec_ns_step_linear_adjoint_f32(const float* what0, const float* that0, const float* mean, const float* ghat, int gbatch, float* lam,
                                        float* mu, float* gbar, void* work, size_t work_bytes, int batch, int nx, int ny, double Lx, double Ly,
                                        double dt, double kappa, double gx, double gy, double bx, double by, const float* lin, int nsteps,
                                        void* stream);
/* nns_spec_ns_step_linear_adjoint_f32 that also differentiates the step in its linear operator, the table lin = l = lambda dt / 2 (restatement:
 * tests/pspec_operator_grad_oracle.py).  With E = exp(l) the Lawson RK4 step s1 = E (w0 + dt/2 N0), s2 = E w0 + dt/2 N1, s3 = E^2 w0 + dt E N2,
 * w1 = E^2 w0 + dt/6 (E^2 N0 + 2 E N1 + 2 E N2 + N3) has, per mode, without any N and without a division by E (a stiff mode is safe),
 *     d s1 / dl = s1     d s2 / dl = E w0     d s3 / dl = s3 + E^2 w0     d w1 / dl = (s3 + E^2 w0) / 3 + 2/3 E (s1 + s2)
 * and a cotangent c of z = D dl gives c conj(D).  With lam the cotangent of w1 and r_S = N'(s_S)^T k_(S+1) that of s_S, both already held by
 * adjoint stages 3, 2, 1, one step adds
 *     (r3 + lam / 3) conj(s3 + E^2 w0)  +  r2 conj(E w0) + 2/3 lam conj(E s2)  +  (r1 + 2/3 conj(E) lam) conj(s1)
 * in the launches of those stages: the same 16 launches per step, five more reads and three read-modify-writes of a compact field.  The steady
 * force, the scalar, the buoyancy and the noise change nothing here (they live in N or after the step); the scalar's E_theta is a constant.
 * lbar: float32 [batch][my1][nx][2], out this sum over the steps of the call, ALWAYS one per grid, overwritten; zero outside the band and at
 * (0, 0).  A grid's lbar does not depend on its batch neighbours, every entry has one owner (no atomics: two runs give the same bits), and
 * nsteps steps in one call are bitwise nsteps calls of one step, last first, summed in that order.  lbar is the sum BEFORE the weight of the
 * cotangent convention (the plain grid sum of real fields, unnormalised rfft2 spectra, a stored mode with ky > 0 standing for itself and its
 * mirror image).  The gradient of a loss L in a table shared by the batch is the unique G [my1][nx][2] with
 *     dL = sum over stored entries (G.re dRe l + G.im dIm l)   for every dl that keeps l(-k) = conj(l(k))   (ky = 0 stores both kx and -kx)
 * that obeys this symmetry itself, so that a gradient step on a valid table gives a valid one.  From T = sum over the grids of lbar it is
 *     G(kx, ky) = 2 T(kx, ky) / (nx ny)   for ky > 0,        G(kx, 0) = (T(kx, 0) + conj(T(-kx, 0))) / (2 nx ny)
 * (nns.periodic.PeriodicSolver.evolve does this with one table multiply per backward).  lbar == NULL: exactly the launches and the results of
 * nns_spec_ns_step_linear_adjoint_f32.  nsteps == 0 zeroes lbar, as gbar.  lam, mu, gbar and every other argument, the workspaces and the
 * errors as there (no allocation, no host synchronisation, capturable). */
int nns_spec_ns_step_operator_adjoint_f32(const float* what0, const float* that0, const float* mean, const float* ghat, int gbatch, float* lam,
                                          float* mu, float* gbar, void* work, size_t work_bytes, int batch, int nx, int ny, double Lx, double Ly,
                                          double dt, double kappa, double gx, double gy, double bx, double by, const float* lin, int nsteps,
                                          void* stream, float* lbar);
/* Forward mode of the flow's step (restatement: tests/pspec_tangent_oracle.py): the Jacobian of nsteps steps applied to a perturbation dw^ that
 * is carried along with the flow, J dw where the adjoint calls give J^T r.  The Lawson RK4 recurrences are linear in (w^, N^), so the tangent
 * of a step is the same four stages on dw^ with the same factors E and
 *     dN_i = -M [u dw_x + v dw_y + du w_x + dv w_y]^ + dg^          (u, v, w_x, w_y of the stage state s_i, the means (U0, V0) in u and v;
 *                                                                    du^ = i ky dw^ / |k|^2, dv^ = -i kx dw^ / |k|^2: no mean flow, no (0, 0) mode)
 * dw^ rides in the step's launches as the scalar does (G fields 4-7, a second Ph field): still 8 launches per step plus one per call.
 * what, dwhat: float32 [batch][my1][nx][2], both advanced in place.  what comes out BITWISE as from the forward call the other arguments name --
 * nns_spec_ns_step_f32 / nns_spec_ns_step_forced_f32 (lin == NULL, amp == NULL; ghat == NULL and drag == 0 take the unforced kernels),
 * nns_spec_ns_step_linear_f32 (lin: its table; nu and drag are then ignored), their stochastic forms (amp, clock, ids all non-NULL; all NULL:
 * no noise, seed ignored) -- the advance of clock included; the kick is additive and independent of the state, so the base takes it and dw^
 * does not.  dghat: the perturbation of the source, float32 [dgbatch][my1][nx][2] with dgbatch = 1 (shared by the batch) or batch, or NULL with
 * dgbatch = 0; it is added where g^ is, in every stage, also under an unforced base.  The linear operator acts on dw^ through the factors:
 * drag, hyperviscosity, hypofriction and beta need nothing further.  Linear in (dwhat, dghat) exactly for powers of two; a grid's result does
 * not depend on its batch neighbours; nsteps steps in one call are bitwise nsteps calls of one step.  Nothing is stored per step.  work:
 * nns_spec_ns_tangent_workspace bytes (12 compacted fields, >= nns_spec_ns_workspace: it also serves every unscalared nns_spec_ns_* call).  No
 * allocation, no host synchronisation (capturable).  Several tangents on one base: nns_spec_ns_step_tangents_f32 below; the tangent of the
 * scalar and the buoyant step: nns_spec_ns_step_scalar_tangent_f32 below (this call has no scalar).  Errors, all before any
 * launch: those of nns_spec_ns_step_linear_f32 (a NULL lin is no error here), plus NNS_ERR_INVALID_ARG for a NULL dwhat and for dgbatch not 0
 * without dghat, 1 or batch with it, and NNS_ERR_WORKSPACE below nns_spec_ns_tangent_workspace. */
int nns_spec_ns_tangent_workspace(int batch, int nx, int ny, size_t* bytes);
int nns_spec_ns_step_tangent_f32(float* what, float* dwhat, const float* mean, const float* ghat, int gbatch, const float* dghat, int dgbatch,
                                 void* work, size_t work_bytes, int batch, int nx, int ny, double Lx, double Ly, double dt, double nu, double drag,
                                 const float* lin, const float* amp, unsigned long long seed, long long* clock, const int* ids, int nsteps,
                                 void* stream);
/* ntan tangents on one base, and what a Lyapunov spectrum needs beside them (restatement: tests/pspec_lyapunov_oracle.py).
 * dwhat: float32 [ntan][batch][my1][nx][2], ntan in [1, 32]; member k is exactly a dwhat of nns_spec_ns_step_tangent_f32 and comes out BITWISE
 * as from that call on a copy of the state, what as from the forward call the other arguments name.  The base's u, v, w_x, w_y of every stage are
 * transformed once for all members: per step 2 + 2 ntan inverse and 1 + ntan forward transforms along y where ntan calls run 4 ntan and
 * 2 ntan, and 1 + ntan passes through a column tile against 2 ntan; still 8 launches per step plus one per call.  No source perturbation per
 * member.  work: nns_spec_ns_tangents_workspace bytes (6 + 6 ntan compacted fields, >= nns_spec_ns_workspace).  No allocation, no host
 * synchronisation (capturable).  Errors, all before any launch: NNS_ERR_INVALID_ARG for a NULL dwhat, then for ntan outside [1, 32], then
 * those of nns_spec_ns_step_tangent_f32 in its order, NNS_ERR_WORKSPACE below nns_spec_ns_tangents_workspace.
 * nns_spec_ns_tangent_gram_f64: out float64 [batch][ntan][ntan], out[b][k][l] = 1/2 sum wt Re(conj(d_k) d_l) / |k|^2 / (nx ny)^2 over the kept
 * stored modes (wt 1 on j = 0, 2 on j > 0): the energy inner product, whose diagonal is E of nns_spec_ns_diag_f32 of each member.  Float64
 * sums in a fixed order, no atomics (two runs give the same bits); both triangles written, bitwise symmetric.
 * nns_spec_ns_tangent_combine_f32: d_k <- sum_{l <= k} coef[b][l][k] d_l in place, coef float64 [batch][ntan][ntan] upper triangular (the
 * lower triangle is not read), every stored entry summed in float64 and rounded once.  With coef = R^-1 of the Cholesky factor of the Gram
 * matrix the two calls are one pass of a Cholesky QR; the ntan x ntan algebra between them is the caller's. */
int nns_spec_ns_tangents_workspace(int batch, int ntan, int nx, int ny, size_t* bytes);
int nns_spec_ns_step_tangents_f32(float* what, float* dwhat, int ntan, const float* mean, const float* ghat, int gbatch, void* work,
                                  size_t work_bytes, int batch, int nx, int ny, double Lx, double Ly, double dt, double nu, double drag,
                                  const float* lin, const float* amp, unsigned long long seed, long long* clock, const int* ids,
                                  int nsteps, void* stream);
int nns_spec_ns_tangent_gram_f64(const float* dwhat, int ntan, double* out, int batch, int nx, int ny, double Lx, double Ly, void* stream);
int nns_spec_ns_tangent_combine_f32(float* dwhat, int ntan, const double* coef, int batch, int nx, int ny, void* stream);
/* Forward mode of the scalar and the buoyant step (restatement: tests/pspec_scalar_tangent_oracle.py): the Jacobian of nsteps steps of the
 * system (w^, theta^) applied to a perturbation (dw^, dtheta^) that is carried along with it, J d where
 * nns_spec_ns_step_scalar_adjoint_f32 and nns_spec_ns_step_linear_adjoint_f32 give J^T r.  The same four stages on (dw^, dtheta^), dw^ with the
 * vorticity's factors (real, or complex from lin) and mask, dtheta^ with the scalar's real E_theta and the mask that keeps (0, 0), and about
 * every stage's own state s_i = (w, theta)_i
 *     dN_w     = -M       [u dw_x + v dw_y + du w_x + dv w_y]^ + dg^ + M (i kx by - i ky bx) dtheta^
 *     dN_theta = -M_theta [u dtheta_x + v dtheta_y + du (theta_x + Gx) + dv (theta_y + Gy)]^
 * (u, v of s_i with the means; du^ = i ky dw^ / |k|^2, dv^ = -i kx dw^ / |k|^2: no mean flow, no (0, 0) mode in dw^; the mean of dtheta is
 * carried unchanged and acts on nothing; the scalar has no source and takes no kick, and neither does the perturbation).  The pair rides in
 * the scalar step's launches (G fields 6-11, Ph fields 2 and 3): still 8 launches per step plus one per call, nothing stored per step.
 * what, that, dwhat, dthat: float32 [batch][my1][nx][2], all advanced in place.  (what, that) come out BITWISE as from the forward call the
 * other arguments name -- nns_spec_ns_step_linear_f32 (lin: its table; nu and drag are then ignored), nns_spec_ns_step_stochastic_f32 (amp,
 * clock, ids all non-NULL; all NULL: no noise, seed ignored), nns_spec_ns_step_buoyant_f32 (b != 0), else nns_spec_ns_step_scalar_f32 -- the
 * advance of clock included.  With b = (0, 0), dwhat comes out bitwise as from nns_spec_ns_step_tangent_f32 on the flow alone.  dghat as there.
 * Linear in (dwhat, dthat, dghat) exactly for powers of two; a grid's result does not depend on its batch neighbours; nsteps steps in one
 * call are bitwise nsteps calls of one step.  work: nns_spec_ns_scalar_tangent_workspace bytes (20 compacted fields, >= every other step's
 * workspace but the adjoints' and nns_spec_ns_tangents_workspace).  No allocation, no host synchronisation (capturable).  Several
 * tangents on one base with a scalar: nns_spec_ns_step_scalar_tangents_f32 below.  Errors, all before any launch: those of the forward call, plus NNS_ERR_INVALID_ARG for a NULL that,
 * dwhat or dthat and for dgbatch not 0 without dghat, 1 or batch with it, and NNS_ERR_WORKSPACE below nns_spec_ns_scalar_tangent_workspace. */
int nns_spec_ns_scalar_tangent_workspace(int batch, int nx, int ny, size_t* bytes);
int nns_spec_ns_step_scalar_tangent_f32(float* what, float* that, float* dwhat, float* dthat, const float* mean, const float* ghat, int gbatch,
                                        const float* dghat, int dgbatch, void* work, size_t work_bytes, int batch, int nx, int ny, double Lx,
                                        double Ly, double dt, double nu, double drag, double kappa, double gx, double gy, double bx, double by,
                                        const float* lin, const float* amp, unsigned long long seed, long long* clock, const int* ids,
                                        int nsteps, void* stream);
/* ntan tangent pairs on one base with a scalar, and the scalar half of their inner product (restatement: tests/pspec_scalar_lyapunov_oracle.py).
 * dwhat, dthat: float32 [ntan][batch][my1][nx][2], ntan in [1, 32]; the other arguments are those of nns_spec_ns_step_scalar_tangent_f32
 * without dghat / dgbatch (no source perturbation per member).  (what, that) come out BITWISE as from the forward call the other arguments name,
 * the advance of clock included, and every member (dwhat[k], dthat[k]) BITWISE as from nns_spec_ns_step_scalar_tangent_f32 on a copy of the
 * state with dghat = NULL: the (0, 0) entry of dthat[k] is carried bit for bit, and with b = (0, 0) dwhat[k] is bitwise
 * nns_spec_ns_step_tangents_f32's member.  The base's three inverse and two forward y-transforms and its two column passes are done once for
 * all members (3 + 3 ntan and 2 + 2 ntan transforms per row where ntan single calls run 7 ntan and 4 ntan); still 8 launches per step plus one
 * per call.  A grid's numbers do not depend on its batch neighbours or on ntan; nsteps steps in one call are bitwise nsteps calls of one step.
 * work: nns_spec_ns_scalar_tangents_workspace bytes: 10 + 10 ntan compacted fields of batch my1 nx complex each (accumulators A, A_theta, dA[ntan],
 * dA_theta[ntan]; G 6 + 6 ntan; Ph 2 + 2 ntan), never below nns_spec_ns_workspace; ntan = 1 is nns_spec_ns_scalar_tangent_workspace.  No
 * allocation, no host synchronisation (capturable).  Errors, all before any launch and in this order: NNS_ERR_INVALID_ARG for a NULL that, dwhat
 * or dthat, then for ntan outside [1, 32], then those of the forward call, then NNS_ERR_WORKSPACE below nns_spec_ns_scalar_tangents_workspace.
 * nns_spec_ns_tangent_variance_gram_f64: out float64 [batch][ntan][ntan], out[b][k][l] = 1/2 sum wt Re(conj(dtheta_k) dtheta_l) / (nx ny)^2 over
 * the stored modes but (0, 0) (wt 1 on j = 0, 2 on j > 0): the variance inner product, whose diagonal is bitwise column 0 of
 * nns_spec_ns_scalar_diag_f32 of each member; bitwise symmetric, fixed order of summation, no atomics.  With nns_spec_ns_tangent_gram_f64 of
 * dwhat it gives the inner product E(dw) + weight 1/2 <dtheta'^2> of the pairs; nns_spec_ns_tangent_combine_f32 serves dwhat and dthat with the
 * one coefficient matrix (two calls; the (0, 0) entries of dthat combine linearly with the rest).  Not built: a source perturbation per
 * member, covariant vectors. */
int nns_spec_ns_scalar_tangents_workspace(int batch, int ntan, int nx, int ny, size_t* bytes);
int nns_spec_ns_step_scalar_tangents_f32(float* what, float* that, float* dwhat, float* dthat, int ntan, const float* mean, const float* ghat,
                                         int gbatch, void* work, size_t work_bytes, int batch, int nx, int ny, double Lx, double Ly, double dt,
                                         double nu, double drag, double kappa, double gx, double gy, double bx, double by, const float* lin,
                                         const float* amp, unsigned long long seed, long long* clock, const int* ids, int nsteps, void* stream);
int nns_spec_ns_tangent_variance_gram_f64(const float* dthat, int ntan, double* out, int batch, int nx, int ny, void* stream);
/* Second-order adjoint of the flow's step (restatement: tests/pspec_second_adjoint_oracle.py): the derivative of the reverse mode in a
 * direction, which is the Hessian-vector product of a loss of the rollout.  With (wbar, gbar) = J^T lam of nns_spec_ns_step_adjoint_f32 /
 * nns_spec_ns_step_linear_adjoint_f32 as a function of the start spectrum w0, the source g^ and the cotangent lam, this call also gives
 *     (dwbar, dgbar) = d/de (wbar, gbar)(w0 + e dw0, g^ + e dg^, lam + e dlam) at e = 0.
 * N is bilinear, so N'(s)^T kappa is linear in s, and the derivative of an adjoint stage is the same operator about the TANGENT stage state,
 * without the mean flow.  With s0..s3 the stage states, d0..d3 the tangent stages of nns_spec_ns_step_tangent_f32, F = conj(E), F2 = conj(E^2)
 * (a real E: E, E^2), N'(s)^T kappa as in nns_spec_ns_step_adjoint_f32 and N'_0(d)^T kappa the same expression with u, v, w_x, w_y of d and zero
 * mean flow, one step is
 *     k4 = dt/6 lam                  dk4 = dt/6 dlam
 *     r  = N'(s3)^T k4               dr  = N'(s3)^T dk4 + N'_0(d3)^T k4      wbar  = F2 (lam + r)    dwbar  = F2 (dlam + dr)
 *     k3 = dt/3 F lam + dt F r       dk3 = dt/3 F dlam + dt F dr
 *     r  = N'(s2)^T k3               dr  = N'(s2)^T dk3 + N'_0(d2)^T k3      wbar += F r             dwbar += F dr
 *     k2 = dt/3 F lam + dt/2 r       dk2 = dt/3 F dlam + dt/2 dr
 *     r  = N'(s1)^T k2               dr  = N'(s1)^T dk2 + N'_0(d1)^T k2      wbar += F r             dwbar += F dr
 *     k1 = dt/6 F2 lam + dt/2 F r    dk1 = dt/6 F2 dlam + dt/2 F dr
 *     r  = N'(s0)^T k1               dr  = N'(s0)^T dk1 + N'_0(d0)^T k1      wbar += r               dwbar += dr
 *     gbar += k1 + k2 + k3 + k4      dgbar += dk1 + dk2 + dk3 + dk4
 * The left column is the adjoint, unchanged: lam and gbar come out BITWISE as from nns_spec_ns_step_adjoint_f32 (lin == NULL) or
 * nns_spec_ns_step_linear_adjoint_f32 without a scalar (lin: the forward's table; nu and drag are then ignored).  A stochastic step is
 * differentiated as the deterministic step it contains: the saved starts carry the kicks, the tangent takes none, the generator never runs.
 * what0, dwhat0: float32 [nsteps][batch][my1][nx][2], the spectrum and its tangent at the start of every step as a forward of
 * nns_spec_ns_step_tangent_f32 in one-step calls saved them; only read.  mean, ghat / gbatch, dghat / dgbatch: that forward's.  lam, dlam:
 * float32 [batch][my1][nx][2], in the cotangent of the state after the last step and its derivative in the direction, out (wbar, dwbar) before
 * the first step; both updated in place.  gbar, dgbar: the same shape, overwritten with the sums over the steps, one per grid; either or both
 * may be NULL.  Per step the stages (s_i, d_i) are recomputed by the tangent step's 7 launches, whose column kernels of stages 1-3 also store
 * them, then 9 adjoint launches carry both quadruples: 16 launches per step, no allocation, no host synchronisation (capturable), no atomics;
 * a grid's result does not depend on its batch neighbours; lam and dlam of nsteps steps in one call are bitwise those of nsteps calls of one
 * step, last first (gbar and dgbar are then the sums of those calls', rounded in another order); linear in (dwhat0, dghat, dlam) exactly for
 * powers of two.  nsteps == 0 zeroes gbar and dgbar.  work: nns_spec_ns_second_adjoint_workspace bytes: 24
 * compacted fields of batch my1 nx complex each (two accumulators that become wbar and dwbar, G 12, Ph 4, the kept stages s1-s3 and d1-d3),
 * never below nns_spec_ns_workspace: >= nns_spec_ns_adjoint_workspace (13) and nns_spec_ns_tangent_workspace (12).  No scalar and no
 * derivative in the table.  Errors, all before any launch and in this order: NNS_ERR_INVALID_ARG for a NULL what0, mean, lam or work or
 * batch < 1, then for a NULL dwhat0 or dlam, then for dt, nu, drag (without lin) or nsteps out of range, then for gbatch, then for dgbatch not 0
 * without dghat, 1 or batch with it; then the box and the axes; then NNS_ERR_WORKSPACE below nns_spec_ns_second_adjoint_workspace. */
int nns_spec_ns_second_adjoint_workspace(int batch, int nx, int ny, size_t* bytes);
int nns_spec_ns_step_second_adjoint_f32(const float* what0, const float* dwhat0, const float* mean, const float* ghat, int gbatch,
                                        const float* dghat, int dgbatch, float* lam, float* dlam, float* gbar, float* dgbar, void* work,
                                        size_t work_bytes, int batch, int nx, int ny, double Lx, double Ly, double dt, double nu, double drag,
                                        const float* lin, int nsteps, void* stream);
/* Lagrangian tracers (csrc/pspec_particles.hip; restatement: tests/pspec_particles_oracle.py): the flow read at points that are no grid
 * nodes, and one Runge-Kutta stage of particle positions.  Interpolation by periodic tensor-product B-splines of order 4 (cubic, 4 x 4 nodes)
 * or 6 (quintic, 6 x 6 nodes) with the exact prefilter in Fourier space: the coefficients of a field f are
 *     c = irfft2[ f^(m_x, m_y) / (beta(2 pi m_x / nx) beta(2 pi m_y / ny)) ],
 *     beta(t) = (2 + cos t) / 3 (order 4),  (66 + 52 cos t + 2 cos 2t) / 120 (order 6);  beta >= 0.5 / 0.325 inside the 2/3 band.
 * A particle at x has cell i = floor(x / hx), hx = Lx / nx, and offset t = x / hx - i, both in float64; the nodes are i-1 .. i+2 (order 4) or
 * i-2 .. i+3 (order 6) modulo nx, likewise in y.  Order-4 weights (1-t)^3/6, (3t^3 - 6t^2 + 4)/6, (-3t^3 + 3t^2 + 3t + 1)/6, t^3/6; order-6
 * weights B5(t - j), j = -2 .. 3, B5 the centred quintic B-spline.  Weights are made in float64 and rounded once to float32; the value is
 * sum_a wx[a] (sum_c wy[c] C[i+a][j+c]), the inner sum an fmaf chain over c ascending from 0, the outer one over a ascending from 0.  One lane
 * per particle, no atomics, no reduction across lanes: a particle's result depends only on its own position and its grid's coefficients, and
 * repeats bitwise.  Every node index is masked with n - 1, so no position, however large, infinite or nan, reads outside its grid (a non-finite
 * position gives a non-finite value).  Positions are float64 [batch][npart][2] = (x, y), UNWRAPPED: only the cell index is taken modulo the box.
 *
 * nns_spec_ns_particle_coefs_f32: coef, float32 [nfields][batch][nx][ny], <- the spline coefficients of the fields named by the mask
 * `fields` (bit 0 u, 1 v, 2 w, 3 theta; nfields = the bits set, stored by ascending bit) of the state (what, mean[, that]): u^ and v^ from w^ as
 * nns_spec_ns_fields_f32 takes them, the mean flow in the (0, 0) coefficient (beta(0) = 1 and the weights sum to 1), theta with its mean.  One
 * pointwise launch and nns_spec_irfft2_f32 over nfields batch grids: the fields() pattern without its pressure solve.  that may be NULL without
 * bit 3.  work: nns_spec_ns_particle_workspace(batch, nfields, nx, ny) = nfields batch nx (ny / 2 + 1) 8 bytes; nothing is kept in it.
 * nns_spec_ns_particle_sample_f32: out, float32 [batch][npart][nfields], <- the splines of coef's nfields (1 .. 4) images at pos.
 * nns_spec_ns_particle_stage_f32: one stage of an explicit Runge-Kutta scheme on coef = the images (u, v), float32 [2][batch][nx][ny]:
 *     k = (u, v)(pos_in), float32 promoted to float64;   s = (first ? 0 : acc) + wk k;
 *     closing == 0:  acc <- s,  pos_out <- pos0 + a k;       closing != 0:  pos_out <- pos0 + c s  (acc is read unless first, never written)
 * every product-sum one float64 fma.  acc, pos0, pos_in, pos_out: float64 [batch][npart][2].  pos_in may alias pos0 or pos_out (a lane reads
 * its particle before it writes it); pos_out may alias pos0 only in the closing stage; acc may be NULL only when first and closing.
 * Classical RK4 over a PAIR of flow steps (H = 2 dt; U_n, U_n+1, U_n+2 the coefficients at the step boundaries, which a Lawson RK4 flow gives
 * exactly: no interpolation in time): (U_n, pos_in = x, a = dt, wk = 1, first), (U_n+1, a = dt, wk = 2), (U_n+1, a = 2 dt, wk = 2),
 * (U_n+2, wk = 1, c = dt / 3, closing, pos_out = x).  Heun over one step: (U_n, a = dt, wk = 1, first), (U_n+1, wk = 1, c = dt / 2, closing).
 * No allocation, no host synchronisation (capturable).
 * Errors, all before any launch and in this order: NNS_ERR_INVALID_ARG for a NULL pointer (coefs: what, mean, coef, work; sample: coef, pos,
 * out; stage: coef, pos0, pos_in, pos_out) or batch < 1; (stage) for a NULL acc unless first and closing, then for pos_out == pos0 in a stage that
 * is not closing; (sample, stage) for npart < 1 or batch npart >= 2^31; for order not 4 or 6; (coefs) for fields not in [1, 15], then for bit 3
 * with a NULL that; (sample) for nfields not in [1, 4]; (stage) for a non-finite a, wk or c; for Lx, Ly not positive and finite; then
 * NNS_ERR_UNSUPPORTED for an axis that is not a power of two in [64, 1024]; then (coefs) NNS_ERR_WORKSPACE below the size query.  The query:
 * NNS_ERR_INVALID_ARG for a NULL bytes or batch < 1, then for nfields not in [1, 4], then NNS_ERR_UNSUPPORTED for the axes. */
int nns_spec_ns_particle_workspace(int batch, int nfields, int nx, int ny, size_t* bytes);
int nns_spec_ns_particle_coefs_f32(const float* what, const float* that, const float* mean, float* coef, int fields, int order, void* work,
                                   size_t work_bytes, int batch, int nx, int ny, double Lx, double Ly, void* stream);
int nns_spec_ns_particle_sample_f32(const float* coef, const double* pos, float* out, int nfields, int order, int batch, long npart, int nx,
                                    int ny, double Lx, double Ly, void* stream);
int nns_spec_ns_particle_stage_f32(const float* coef, const double* pos0, const double* pos_in, double* pos_out, double* acc, double a,
                                   double wk, double c, int first, int closing, int order, int batch, long npart, int nx, int ny, double Lx,
                                   double Ly, void* stream);
/* Reverse mode of the sampling (csrc/pspec_particles.hip; restatement: tests/pspec_particles_adjoint_oracle.py): the transpose of the gather
 * as a sorted spread without floating-point atomics, the transpose of the coefficient build, and the derivative of a sample in the position.
 *
 * nns_spec_ns_particle_cells_i32: key, int32 [batch][npart], <- (b nx + ci) ny + cj, (ci, cj) the wrapped cell of the particle as the gather
 * finds it (the same float64 floor, the same mask: any position, +-inf and nan included, gives a key inside its own grid).  The caller sorts
 * the keys STABLY (the particles of a cell stay in ascending index, which fixes the order of summation below) and takes perm, int64
 * [batch npart] = the particle (an index into [batch][npart]) of every sorted slot, and start, int32 [batch nx ny + 1] = the first slot of
 * every cell and, last, batch npart (torch.sort and torch.searchsorted on the device; neither synchronises the host).
 * nns_spec_ns_particle_spread_f32: cbar, float32 [nfields][batch][nx][ny], <- the transpose of nns_spec_ns_particle_sample_f32 applied to
 * cot, float32 [batch][npart][nfields]: cbar[f][b][i0 + a][j0 + c] = sum_p wx_p[a] wy_p[c] cot[b][p][f].  Gather form: a staging launch (one
 * lane per sorted slot) writes a record (wx, wy, cot) per slot into work, the forward's weights (float64, rounded once); a node launch (one
 * lane per node) visits the order x order cells whose stencil covers the node, ci = i - a + order / 2 - 1, cj = j - c + order / 2 - 1 modulo
 * the axis, a ascending, then c ascending, then the cell's slots ascending; wx[a] wy[c] is one float32 multiply, every term one float64 fma
 * into one float64 accumulator per field, rounded once on store.  Every node is written (zero where no particle reaches: cbar need not be
 * cleared); no atomics, so two runs give the same bits and a grid does not depend on its batch neighbours.  perm entries outside
 * [0, batch npart) contribute nothing and start is clamped to [0, batch npart]: a wrong table reads nothing outside the buffers.
 * work: nns_spec_ns_particle_spread_workspace(batch, npart, order) = batch npart (2 order + 4) 4 bytes.
 * nns_spec_ns_particle_sample_grad_f32: grad, float32 [batch][npart][nfields][2], <- (d/dx, d/dy) of the splines of coef at pos: the gather of
 * nns_spec_ns_particle_sample_f32 with derivative weights on one axis, (1 / hx) sum_a wx'[a] (sum_c wy[c] C) and (1 / hy) sum_a wx[a]
 * (sum_c wy'[c] C), the same fmaf chains (c ascending inside a ascending), the division in float64.  Order-4 derivative weights -(1-t)^2/2,
 * (3t^2 - 4t)/2, (-3t^2 + 2t + 1)/2, t^2/2; order 6: B5'(t - j) piece by piece; float64, rounded once.  The splines are C^2 (C^4), so the
 * derivative is continuous across cells.
 * nns_spec_ns_particle_coefs_adjoint_f32: the transpose of nns_spec_ns_particle_coefs_f32 as a map between physical fields.  cbar, float32
 * [nfields][batch][nx][ny]: the cotangents of the coefficient images of the mask `fields`, by ascending bit.  wbar_hat (and thbar_hat with bit
 * 3), float32 [batch][my1][nx][2] in the layout of what, <- with c^ = nns_spec_rfft2_f32(cbar) inside the 2/3 band
 *     wbar_hat = [(-i ky c_u^ + i kx c_v^) / |k|^2 + c_w^] / (beta_x beta_y), (0, 0) zero;     thbar_hat = c_theta^ / (beta_x beta_y), (0, 0) kept
 * the forward's multipliers conjugated (the map is real); the unnormalised transform here stands where the forward's 1 / (nx ny) inverse
 * stood, so nns_spec_ns_scalar_field_f32 of wbar_hat is the cotangent of the vorticity field that init_vorticity took.  The mean flow gets no
 * cotangent.  wbar_hat may be NULL without bits 0-2, thbar_hat without bit 3.  work: nns_spec_ns_particle_workspace(batch, nfields, nx, ny).
 * No allocation, no host synchronisation (capturable).
 * Errors, all before any launch and in this order: (1) NNS_ERR_INVALID_ARG for a NULL pointer (cells: pos, key; spread: cot, pos, perm, start,
 * cbar, work; sample_grad: coef, pos, grad; coefs_adjoint: cbar, work) or batch < 1; (2) (cells, spread, sample_grad) for npart < 1 or batch
 * npart >= 2^31; (3) (spread, sample_grad, coefs_adjoint) for order not 4 or 6; (4) (spread, sample_grad) for nfields not in [1, 4],
 * (coefs_adjoint) for fields not in [1, 15], then for a NULL wbar_hat with bits 0-2, then a NULL thbar_hat with bit 3; (5) for Lx, Ly not
 * positive and finite; (6) NNS_ERR_UNSUPPORTED for an axis that is not a power of two in [64, 1024], then (cells, spread) for batch nx ny >=
 * 2^31; (7) (spread, coefs_adjoint) NNS_ERR_WORKSPACE below the size query.  The spread's query: NNS_ERR_INVALID_ARG for a NULL bytes or
 * batch < 1, then for npart, then for order. */
int nns_spec_ns_particle_cells_i32(const double* pos, int* key, int batch, long npart, int nx, int ny, double Lx, double Ly, void* stream);
int nns_spec_ns_particle_spread_workspace(int batch, long npart, int order, size_t* bytes);
int nns_spec_ns_particle_spread_f32(const float* cot, const double* pos, const long long* perm, const int* start, float* cbar, int nfields,
                                    int order, void* work, size_t work_bytes, int batch, long npart, int nx, int ny, double Lx, double Ly,
                                    void* stream);
int nns_spec_ns_particle_sample_grad_f32(const float* coef, const double* pos, float* grad, int nfields, int order, int batch, long npart,
                                         int nx, int ny, double Lx, double Ly, void* stream);
int nns_spec_ns_particle_coefs_adjoint_f32(const float* cbar, float* wbar_hat, float* thbar_hat, int fields, int order, void* work,
                                           size_t work_bytes, int batch, int nx, int ny, double Lx, double Ly, void* stream);

/* ---- neural_spectral field predictor: src/neural_spectral/spectral_ode.py, anode/ ------------ */
enum { NNS_ODE_EULER = 0, NNS_ODE_RK2 = 1, NNS_ODE_RK4 = 2 };   /* anode/scheme.py:21-42 */
/* ODEFunc (spectral_ode.py:14-34: Linear(K,hidden)-ReLU-Linear(hidden,hidden)-ELU-Linear(hidden,K), torch
 * nn.Linear layout W [out][in]) integrated by odesolver (anode/odesolver.py:21-37, time_stepper.py:35-45):
 * dt = 1/Nt, out[n] = y_{n+1} for n = 0..Nt-1, out is [Nt, mb, K].  One persistent kernel: weights resident
 * in LDS, linears on f32-input MFMA.  hidden must be 128, K <= 32. */
int nns_ode_mlp_fwd_f32(const float* z0, const float* W0, const float* b0, const float* W1, const float* b1,
                        const float* W2, const float* b2, float* out, int mb, int K, int hidden, int Nt,
                        int method, void* stream);
/* Backward of the above (what Checkpointing_Adjoint.backward computes, anode/adjoint.py:52-70, by
 * recomputation): given states = the forward's out and grad_out [Nt, mb, K], writes grad_z0 [mb, K] and the six
 * parameter gradients (zeroed and accumulated inside the call).  work: nns_ode_mlp_bwd_workspace(mb) bytes. */
size_t nns_ode_mlp_bwd_workspace(int mb);
int nns_ode_mlp_bwd_f32(const float* z0, const float* W0, const float* b0, const float* W1, const float* b1,
                        const float* W2, const float* b2, const float* states, const float* grad_out,
                        float* grad_z0, float* gW0, float* gb0, float* gW1, float* gb1, float* gW2, float* gb2,
                        void* work, int mb, int K, int hidden, int Nt, int method, void* stream);
/* The time-parallel form of that backward (anode/adjoint.py:38-70 walks the steps backwards one by one; every step's Jacobian
 * depends only on its own stored input state, so all of them can be formed at once):
 *   nns_ode_mlp_bwd_steps_f32  backward of `rows` INDEPENDENT single steps y -> y' of size dt: grad_y[r] = (dy'/dy)^T grad_out[r],
 *                              parameter gradients summed over the rows (work: nns_ode_mlp_bwd_workspace(rows) bytes); the six
 *                              parameter-gradient pointers may ALL be NULL (pass 1 below wants grad_y only: their products, the
 *                              zero-fills and the atomics are then skipped);
 *   nns_ode_adjoint_chain_f32  lam[Nt-1] = g[Nt-1], lam[s-1] = g[s-1] + lam[s] J[s]: the adjoint recurrence on the K x K step
 *                              Jacobians J [Nt][mb][K][K] (K <= 64), g, lam [Nt][mb][K].
 * Pass 1: rows (s, b, i) with grad_out = e_i give J; chain; pass 2: rows (s, b) with grad_out = lam[s][b] give the parameter
 * gradients and grad_z0 = grad_y of step 0 -- three launches of parallel work instead of Nt dependent steps. */
int nns_ode_mlp_bwd_steps_f32(const float* y, const float* W0, const float* b0, const float* W1, const float* b1, const float* W2,
                              const float* b2, const float* grad_out, float* grad_y, float* gW0, float* gb0, float* gW1, float* gb1,
                              float* gW2, float* gb2, void* work, int rows, int K, int hidden, double dt, int method, void* stream);
int nns_ode_adjoint_chain_f32(const float* J, const float* g, float* lam, int Nt, int mb, int K, void* stream);
/* Basis expansion (PDEFunc.forward, spectral_ode.py:71-79): pred[t][c][p] = sum_k coeff[t][k][c] basis[k][c][p];
 * coeff [T, K, C] (T = nt*mb), basis [K, C, P] (P = nx*ny), pred [T, C, P].  K <= 32. */
int nns_basis_expand_f32(const float* coeff, const float* basis, float* pred, int T, int K, int C, int P, void* stream);
/* Backward of nns_basis_expand_f32 for an arbitrary upstream gradient grad_pred [T, C, P]: gcoeff [T, K, C]
 * (zeroed inside, atomics), gbasis [K, C, P]. */
int nns_basis_expand_bwd_f32(const float* coeff, const float* basis, const float* grad_pred, float* gcoeff,
                             float* gbasis, int T, int K, int C, int P, void* stream);
/* Fused training loss (spectral_ode.py:182, torch.norm(pred - obs, 2)): accumulates sum (pred-obs)^2 into the
 * device double *sumsq (caller zeroes it; loss = sqrt) without materialising pred; obs is read once. */
int nns_basis_loss_fwd_f32(const float* coeff, const float* basis, const float* obs, double* sumsq,
                           int T, int K, int C, int P, void* stream);
/* Its gradients for g = scale * (pred - obs): gcoeff [T, K, C] (zeroed inside, atomics) and gbasis [K, C, P]. */
int nns_basis_loss_bwd_f32(const float* coeff, const float* basis, const float* obs, float scale,
                           float* gcoeff, float* gbasis, int T, int K, int C, int P, void* stream);
/* Loss and gradient in ONE sweep over the observations (training step, spectral_ode.py:178-190: forward, loss.backward()):
 * *sumsq += sum (pred - obs)^2 (zeroed by the caller) and gcoeff / gbasis = d(sumsq / 2) / d(coeff, basis), i.e. the gradient
 * WITHOUT the upstream / loss factor, which the caller applies afterwards (the gradient is linear in it).  obs, the only
 * large stream, is read once instead of twice. */
int nns_basis_loss_fused_f32(const float* coeff, const float* basis, const float* obs, double* sumsq, float* gcoeff, float* gbasis,
                             int T, int K, int C, int P, void* stream);

/* Per-pixel MLP forward (BasisFunc, spectral_ode.py:100-119: a stack of 1x1 Conv2d with ReLU between layers,
 * generalised to <= 8 layers of width <= 64): x [mb, widths[0], P] -> y [mb, widths[nlayers], P], P = nx*ny.
 * weights / biases: the layers' [C_out][C_in] matrices and [C_out] vectors packed back to back (device);
 * widths_host: nlayers+1 ints (host).  All layers are chained in MFMA accumulators (no LDS/HBM round trip
 * between layers).  bf16 == 0: float32 MFMA (exact fp32); bf16 != 0: bfloat16 operands, float32 accumulate. */
int nns_pixel_mlp_fwd_f32(const float* x, const float* weights, const float* biases, float* y, int mb, int P,
                          const int* widths_host, int nlayers, int bf16, void* stream);

/* Its backward (what autograd would do for the reference's Conv2d/ReLU stack, spectral_ode.py:100-119), fused in one
 * launch that recomputes the forward in registers: gy [mb, widths[nlayers], P] -> gx [mb, widths[0], P], gW / gB packed
 * like weights / biases (overwritten).  bf16 != 0: operands rounded to bfloat16 exactly as the forward does, float32
 * accumulation, any supported shape; bf16 == 0: float32 operands (v_mfma_f32_32x32x2_f32), widths <= 32 only (wider:
 * NNS_ERR_UNSUPPORTED).  Weight gradients contract over pixels through LDS images and are reduced over workgroups in a
 * fixed order.  workspace: nns_pixel_mlp_bwd_workspace bytes of device memory. */
int nns_pixel_mlp_bwd_workspace(const int* widths_host, int nlayers, size_t* bytes);
int nns_pixel_mlp_bwd_f32(const float* x, const float* gy, const float* weights, const float* biases,
                          float* gx, float* gW, float* gB, int mb, int P, const int* widths_host, int nlayers, int bf16,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ---- chorin_spectral (Chebyshev collocation): src/chorin_spectral/simulate.py ---------------- */
/* Row-major float64 GEMM on the matrix cores: C = alpha * op(A) op(B) + beta * C, op = transpose when the flag is
 * set; `batch` independent problems stored back to back.  Replaces the `@` products of _predictor_step
 * (:264-298) and _correction_step (:361-380). */
int nns_cheb_gemm_f64(const double* A, int lda, int transA, const double* B, int ldb, int transB, double* C, int ldc,
                      int M, int N, int K, double alpha, double beta, int batch, void* stream);
/* F = 2 f - 3 dt (un fx + vn fy) + dt (un1 f1x + vn1 f1y) + dt (fxx + fyy), elementwise on n values (:277-282). */
int nns_cheb_helmholtz_rhs_f64(const double* f, const double* un, const double* vn, const double* un1, const double* vn1,
                               const double* fx, const double* fy, const double* f1x, const double* f1y,
                               const double* fxx, const double* fyy, double* F, int n, double dt, void* stream);
/* out[i][j] = Hm[i][j] / (c0 + cx * lam_x[i] + cy * lam_y[j])  (:287-288, :372-373). */
int nns_cheb_diag_div_f64(const double* Hm, const double* lam_x, const double* lam_y, double* out, int ni, int nj,
                          double c0, double cx, double cy, void* stream);
/* full [Nx, Ny] = interior sol [(Nx-2), (Ny-2)] + boundary rows x0, xN [Ny-2] and columns y0, yN [Nx-2], corners 0
 * (:322-334). */
int nns_cheb_embed_f64(const double* sol, const double* x0, const double* xN, const double* y0, const double* yN,
                       double* full, int Nx, int Ny, void* stream);

/* ---- slab decomposition of one grid over the GPUs of a node: device-side message packing (nns/slab.py) --------------
 * No reference counterpart (src/neural_spectral/spectral_ode.py:155-156 runs on one device); SURVEY.md section 8 (e).
 * fields_host: a HOST array of nfields (<= 4) device pointers.  One launch each.
 * gather:  msg[f][o][e] = fields[f][o * outer_stride + line_off + e * elem_stride],  o < nouter, e < len;  scatter: the reverse.
 *   (a row of [B][nloc][ny] slabs: nouter = B, outer_stride = nloc * ny, line_off = row * ny, len = ny, elem_stride = 1;
 *    a column of an [nx][nyl] slab: nouter = 1, line_off = column, len = nx, elem_stride = nyl) */
int nns_slab_gather_lines_f32(const float* const* fields_host, int nfields, float* msg, long nouter, long outer_stride, long line_off,
                              long len, long elem_stride, void* stream);
int nns_slab_gather_lines_f64(const double* const* fields_host, int nfields, double* msg, long nouter, long outer_stride, long line_off,
                              long len, long elem_stride, void* stream);
int nns_slab_scatter_lines_f32(const float* msg, float* const* fields_host, int nfields, long nouter, long outer_stride, long line_off,
                               long len, long elem_stride, void* stream);
int nns_slab_scatter_lines_f64(const double* msg, double* const* fields_host, int nfields, long nouter, long outer_stride, long line_off,
                               long len, long elem_stride, void* stream);
/* transpose_pack: row slabs fields[f][b][i][j] -> send[d][f][b][i][jj], d = j / (ny / nranks): the all-to-all send buffer with every
 * destination's column block contiguous; transpose_unpack: recv[s][f][b][i][jj] -> fields[f][b][i][s * (ny / nranks) + jj]. */
int nns_slab_transpose_pack_f32(const float* const* fields_host, int nfields, float* send, int batch, int nloc, int ny, int nranks, void* stream);
int nns_slab_transpose_pack_f64(const double* const* fields_host, int nfields, double* send, int batch, int nloc, int ny, int nranks, void* stream);
int nns_slab_transpose_unpack_f32(const float* recv, float* const* fields_host, int nfields, int batch, int nloc, int ny, int nranks, void* stream);
int nns_slab_transpose_unpack_f64(const double* recv, double* const* fields_host, int nfields, int batch, int nloc, int ny, int nranks, void* stream);
/* transpose_pack of the batch chunk [grid0, grid0 + batch) of row slabs fields[f] [batch_total][nloc][ny] into send [d][f][batch][nloc][ny / nranks]
 * AND, in the same launch, the halo messages of the WHOLE local batch: first[f][b][j] = fields[f][b][0][j], last[f][b][j] = fields[f][b][nloc-1][j],
 * b < batch_total (first = last = NULL: the pack alone).  One launch where the slab step had three (round 4).  Needs 16-byte aligned pointers and
 * ny / nranks a multiple of the 16-byte vector (NNS_ERR_UNSUPPORTED otherwise: use the separate calls). */
int nns_slab_pack_halo_f32(const float* const* fields_host, int nfields, float* send, float* first, float* last, int batch_total, int grid0, int batch,
                           int nloc, int ny, int nranks, void* stream);
int nns_slab_pack_halo_f64(const double* const* fields_host, int nfields, double* send, double* first, double* last, int batch_total, int grid0, int batch,
                           int nloc, int ny, int nranks, void* stream);

/* ---- loss head of the physics-informed training step (the hypothesis of
 * src/neural_spectral/derivations/derivation.tex:25-34, which the reference states and never implements) ----------------------------------
 *   pred = state + mlp_out (channels u, v, p);  data = mean (pred - target)^2;  phys = mean r_u^2 + mean r_v^2 + w_div mean r_div^2 of the
 *   residual of pred;  total = data + lam phys.   Three HBM-bound passes replace the tensor ops between the MLP and the residual kernels
 *   (csrc/pinn_kernels.hip); the sums are deterministic (fixed grid, partials in double added in index order).
 * workspace: nns_pinn_workspace_bytes() bytes of device memory, 8-byte aligned, ZEROED ONCE by the caller (the kernels leave it reusable),
 * one per stream in flight. */
long nns_pinn_workspace_bytes(void);
/* assemble: out, state, target [batch][3][npix] (target NULL: no data term) -> u, v, p [batch][npix] = the channels of state + out;
 * u_prev, v_prev [batch][npix] = channels 0, 1 of state (both NULL when the caller already has them contiguous: batch = 1); the data term's
 * sum of squares stays in the workspace for nns_pinn_loss_f32. */
int nns_pinn_assemble_f32(const float* out, const float* state, const float* target, float* u, float* v, float* p, float* u_prev, float* v_prev,
                          void* workspace, int batch, long npix, void* stream);
/* loss: the residual fields r_u, r_v, r_div (n values each) of the assembled prediction -> out3 (device) = (total, data, phys); n_data = the
 * number of values under the data mean (3 batch npix; 0: no target).  When w_div != 1, r_div is SCALED IN PLACE by w_div so that the residual
 * adjoint applied to (r_u, r_v, r_div) as they stand gives (n / 2) d phys / d (u, v, p). */
int nns_pinn_loss_f32(const float* r_u, const float* r_v, float* r_div, long n, void* workspace, double n_data, double lam, double w_div, float* out3,
                      void* stream);
/* combine: grad_out [batch][3][npix] = up_data[0] c_data (pred - target) + up_phys[0] c_phys (g_u, g_v, g_p), pred = (u, v, p) [batch][npix],
 * (g_u, g_v, g_p) = the residual adjoint's output; up_* are DEVICE scalars (autograd's upstream gradient: no host read-back), c_data = 2 / n_data,
 * c_phys = 2 lam / n.  target NULL: the physics part alone (u, v, p, up_data unused). */
int nns_pinn_combine_f32(const float* g_u, const float* g_v, const float* g_p, const float* u, const float* v, const float* p, const float* target,
                         const float* up_data, const float* up_phys, double c_data, double c_phys, float* grad_out, int batch, long npix, void* stream);

/* ---- optimiser step (src/neural_spectral/spectral_ode.py:171,189; spectral_ode2.py:159,171; rnn.py:90,102; spectral_rnn.py:131,149:
 * torch.optim.Adam(model.parameters(), lr=1e-3) ... optimizer.step()) as ONE launch over all parameter tensors -------------------------------
 * Tables of ntensors device pointers (host arrays) and element counts; float32, contiguous; exp_avg / exp_avg_sq are the optimiser state, updated
 * in place like the parameters.  Arithmetic in torch's order (no amsgrad): g = grad (+ weight_decay p; maximize: -grad), m += (1 - beta1)(g - m),
 * v = beta2 v + (1 - beta2) g g, p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps); `step` counts from 1. */
int nns_adam_step_f32(float* const* params_host, const float* const* grads_host, float* const* exp_avg_host, float* const* exp_avg_sq_host,
                      const long* sizes_host, int ntensors, double lr, double beta1, double beta2, double eps, double weight_decay, long step,
                      int maximize, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NNS_H */
