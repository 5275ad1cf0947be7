"""Edge cases of the multigrid pressure solve (tests/test_gpu_multigrid_edges.py runs them on the GPU against tests/mg_oracle.py;
tests/test_oracle_multigrid.py shows on the CPU which launch path each takes and that their bounds would catch a wrong operator).

Which kernels run depends on the shape and the element size (mg_oracle.tail_level, the host split of csrc/mg_kernels.hip):
  'single'  min(nx, ny) <= 9: one level, mg_tail_kernel does one exact sine-basis solve per cycle
  'lds'     tail 0: the whole V-cycle in one workgroup's LDS, one launch per cycle
  'mixed'   tail >= 1: the fine levels chip-wide (mg_smooth / restrict / prolong / norm / finish), the coarser ones in the LDS tail
"""
import mg_oracle as M


def _eq(nx, ny):
    """Equal spacing on both axes, the longer axis spanning 2."""
    h = 2.0 / (max(nx, ny) - 1)
    return h, h


def _box(nx, ny):
    """The chorin_fd spacings, [-1, 1]^2 (aspect (nx - 1) / (ny - 1) at the finest level)."""
    return M.spacings(nx, ny)


# (nx, ny, B, dx, dy), reason
CASES = [
    # single level
    ((5, 5, 3) + _eq(5, 5), 'smallest grid: 3 x 3 unknowns'),
    ((9, 9, 2) + _eq(9, 9), 'largest square that does not coarsen'),
    ((5, 33, 2) + _eq(5, 33), 'single level, a 33-node axis (the largest sine table) on axis 1'),
    ((33, 9, 2) + _eq(33, 9), 'single level, a 33-node axis on axis 0'),
    # all in LDS (tail 0)
    ((17, 17, 2) + _eq(17, 17), 'two levels'),
    ((33, 33, 2) + _eq(33, 33), 'three nested levels'),
    ((84, 84, 1) + _eq(84, 84), 'the largest float64 square in LDS: 147.7 KB'),
    ((119, 119, 1) + _eq(119, 119), 'the largest float32 square in LDS: 148.6 KB (float64: tail 1)'),
    ((129, 33, 2) + _eq(129, 33), 'non-square box, coarsest 33 x 9'),
    ((33, 129, 2) + _eq(33, 129), 'non-square box, coarsest 9 x 33'),
    ((65, 65, 2, 2.0 / 64, 1.0 / 64), 'cell aspect exactly 2 on every level'),
    # around the LDS limits
    ((85, 85, 1) + _eq(85, 85), 'first float64 square past the limit: float32 tail 0, float64 tail 1'),
    ((120, 120, 1) + _eq(120, 120), 'first float32 square past the limit: tail 1 in both types'),
    # mixed
    ((200, 200, 1) + _eq(200, 200), 'float32 tail 1, float64 tail 2, non-nested levels'),
    ((257, 65, 1) + _eq(257, 65), 'non-square box, one chip-wide level, coarsest 33 x 9'),
    ((1025, 1024, 1) + _eq(1025, 1024), 'axis 0 nested, axis 1 not: the aspect drifts to 1.14 on the coarsest level'),
    ((1000, 600, 1) + _box(1000, 600), '[-1, 1]^2 box: aspect 1.67 .. 1.75, float32 tail 3, float64 tail 4'),
]


def case_id(c):
    nx, ny, B, dx, dy = c
    return '%dx%dxB%d' % (nx, ny, B) + ('' if dx == dy else '_dx%.3gdy' % (dx / dy))


def problem(case):
    """The case's float64 problem (p, C), [B, nx, ny]: a random boundary ring, a zero interior, a random right-hand side."""
    nx, ny, B = case[:3]
    return M.random_problem(nx, ny, seed=nx * 7 + ny + B, B=B)


def path(nx, ny, elem_size):
    """'single', 'lds' or 'mixed': the launch path of an nx x ny solve with elements of elem_size bytes."""
    if len(M.levels(nx, ny)) == 1:
        return 'single'
    return 'lds' if M.tail_level(nx, ny, elem_size) == 0 else 'mixed'


def cycles_checked(nx, ny):
    """Cycle counts compared with the float64 restatement (k <= 2 on the largest grids: the restatement is the slow part)."""
    return (1, 2, 5) if nx * ny <= 300 * 300 else (1, 2)


# (nx, ny, dx, dy, refused): shapes and spacings whose refusal (NNS_ERR_UNSUPPORTED) must agree with mg_oracle.hierarchy
SHAPE_CHECKS = [
    (1024, 1025, 1.9 * 2.0 / 1024, 2.0 / 1024, True),        # aspect 1.96 at level 5 (32 x 33), 2.02 at level 6 (16 x 17)
    (1024, 1025, 1.7 * 2.0 / 1024, 2.0 / 1024, False),       # the same drift stays below 2 (1.94 at level 7, 9 x 8)
    (1025, 1024) + _eq(1025, 1024) + (False,),
    (65, 65, 2.0 / 64, 1.0 / 64, False),                      # exactly 2
    (65, 65, 2.0 / 64 * (1 + 1e-12), 1.0 / 64, True),         # just above 2
    (64, 64, 1.0, 0.3, True),                                 # aspect 3.3 on the finest level
    (1000, 600) + _box(1000, 600) + (False,),
    (600, 1000) + _box(600, 1000) + (False,),
    (4, 64, 0.1, 0.1, True),                                  # 4 nodes on an axis
    (5, 33) + _eq(5, 33) + (False,),
    (5, 34) + _eq(5, 34) + (True,),                           # coarsest (one level) 5 x 34
    (34, 9) + _eq(34, 9) + (True,),
    (1024, 64, 0.01, 0.01, True),                             # coarsest 128 x 8
]

# (nx, ny, B, dtype): batches whose launches span several blocks of 256 grids (mg_init / mg_finish) or, above 1024 grids, one norm and one
# smoothing block per grid
BATCH_CASES = [(64, 64, 300, 'float64'), (64, 64, 300, 'float32'), (129, 129, 300, 'float64'), (129, 129, 300, 'float32'),
               (129, 129, 1100, 'float32')]

# rel-L2 bounds of the float32 solver after k cycles against the float64 restatement started from the float32-rounded p and C, per launch
# path and k.  Measured on the MI355X, worst case over CASES: k = 1 single 2.0e-7 (33x9), lds 2.4e-7 (84x84), mixed 4.5e-7 (1025x1024);
# k = 2 lds 3.2e-6 (85x85), mixed 4.6e-5 (1000x600; 6.3e-6 at 1025x1024).  The k = 2 errors are float32 rounding: the restatement run in
# NumPy float32 lands at 4.0e-6 (85x85), 4.1e-6 (1025x1024) and 4.1e-5 (1000x600, whose anisotropic cells converge slowest).
# Margins 2.5x, 4.2x, 3.4x; 3.1x, 2.2x.  float64 measured at most 1.1e-14 (BOUND_F64 1e-11, as tests/test_gpu_multigrid.py).
BOUND_F32 = {('single', 1): 5e-7, ('lds', 1): 1e-6, ('mixed', 1): 1.5e-6, ('lds', 2): 1e-5, ('mixed', 2): 1e-4}
BOUND_F64 = 1e-11
