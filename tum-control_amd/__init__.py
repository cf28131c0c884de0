"""
tum-control_amd -- MI355X-native batched SQP-RTI solver behind the AcadosOcpSolver surface used by
bzarr/TUM-CONTROL's NMPC controllers (drop-in for `acados_solver.solve()` and nothing else).

  csrc/            hand-written HIP (gfx950) kernels + the C-ABI (include/tum_nmpc.h) -> libtumnmpc.so
  solver.py        ctypes binding with acados method names (BatchedOcpSolver)
  nmpc.py / snmpc.py / r2nmpc.py   mirrors of the reference's three controller classes (same names, arguments, returns)
  planner.py, closed_loop.py        the producer (PlannerEmulator) and the consumer (plant + estimator) of the solve
  bo.py            Bayesian optimisation of the weight sets (bo_optimize.py): surrogate models, acquisition on the device, candidate selection
  workloads.py, sharding.py         synthetic batches of the BASELINE configs and their group-aligned multi-GPU layout
  config.py        EDGAR vehicle / tyre / MPC constants
"""
__version__ = "0.1.0"
