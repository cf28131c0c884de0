"""CPU-side tests: planner restatement vs golden vectors, workloads, sharding (incl. a world_size-2
gloo run), and the C-ABI surface of the built library (no compute without a GPU)."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_planner_matches_reference_golden(golden_dir):
    from tum_control_amd.planner import load_track, planner_emulator
    g = np.load(os.path.join(golden_dir, "planner.npz"))
    for t in ("monteblanco", "lvms", "modena"):
        tr = load_track(t)
        for i, p in enumerate(g[t + "_pose"]):
            c, r = planner_emulator(tr, p, 39, 3.04)
            assert c == g[t + "_idx"][i]
            np.testing.assert_allclose(r, g[t + "_n39"][i], rtol=0, atol=1e-12)
            c, r = planner_emulator(tr, p, 41, 3.2)
            np.testing.assert_allclose(r, g[t + "_n41"][i], rtol=0, atol=1e-12)


def test_planner_matches_kat_yref(golden_dir):
    from tum_control_amd.planner import load_track, planner_emulator
    d = np.load(os.path.join(golden_dir, "kat0.npz"))
    for i in (0, 30):
        tr = load_track(str(d["track"][i]))
        _, r = planner_emulator(tr, d["x0"][i][:2], 39, 3.04)
        np.testing.assert_allclose(r, d["yref"][i], atol=1e-12)


def test_workloads_deterministic_and_shaped():
    from tum_control_amd.workloads import nominal_batch, scenario_batch
    x0, yref = nominal_batch(16, N=40)
    x0b, yrefb = nominal_batch(16, N=40)
    assert x0.shape == (16, 8) and yref.shape == (16, 41, 6)
    assert np.array_equal(x0, x0b) and np.array_equal(yref, yrefb)
    assert (x0[:, 3] >= 1.0).all() and (yref[:, :, 4:] == 0).all()
    off = np.zeros((3, 8)); off[:, 3] = [0.1, -0.2, 0.3]
    xs, ys, g = scenario_batch(4, off, N=38)
    assert g == 4 and xs.shape == (16, 8) and ys.shape == (16, 39, 6)
    assert np.array_equal(ys[0], ys[3]) and np.allclose(xs[1] - xs[0], off[0])


def test_shard_ranges_partition():
    from tum_control_amd.sharding import shard_range, shard_sizes
    for total, world in ((131072, 8), (32768, 8), (10, 3), (7, 8), (4096, 1)):
        rs = [shard_range(total, world, r) for r in range(world)]
        assert rs[0][0] == 0 and rs[-1][1] == total
        assert all(rs[i][1] == rs[i + 1][0] for i in range(world - 1))
        assert sum(shard_sizes(total, world)) == total
        assert max(shard_sizes(total, world)) - min(shard_sizes(total, world)) <= 1


def test_group_sharding_never_splits_a_scenario_group():
    """ranks own whole scenario groups (a pose with its sigma points / Monte-Carlo draws)."""
    from tum_control_amd.sharding import shard_groups
    for n_groups, gsz, world in ((8192, 16, 8), (1024, 16, 1), (7, 16, 3), (5, 11, 8), (32768, 1, 8)):
        sh = [shard_groups(n_groups, gsz, world, r) for r in range(world)]
        assert sh[0][0] == 0 and sh[0][2] == 0 and sh[-1][1] == n_groups and sh[-1][3] == n_groups * gsz
        for r in range(world):
            g_lo, g_hi, b_lo, b_hi = sh[r]
            assert b_lo == g_lo * gsz and b_hi == g_hi * gsz and b_lo % gsz == 0 and b_hi % gsz == 0
            if r:
                assert sh[r - 1][1] == g_lo and sh[r - 1][3] == b_lo
        # every instance of a group lands on the rank that owns the group
        owner = np.empty(n_groups * gsz, dtype=int)
        for r, (_, _, b_lo, b_hi) in enumerate(sh):
            owner[b_lo:b_hi] = r
        assert (owner.reshape(n_groups, gsz) == owner.reshape(n_groups, gsz)[:, :1]).all()


@pytest.mark.parametrize("cid", [3, 4, 5])
def test_config_workloads_are_shard_invariant(cid):
    """The union of the shards of any world size IS the unsharded batch (per-group random streams keyed by the global
    group index), groups share one yref, and the scenario offsets have the configured statistics."""
    from tum_control_amd import config
    from tum_control_amd.sharding import shard_groups
    from tum_control_amd.workloads import CONFIGS, config_groups
    G, N = 12, 10
    gsz = CONFIGS[cid]["group"]
    x0, yref, g = config_groups(cid, 0, G, G, N=N)
    assert g == gsz and x0.shape == (G * gsz, 8) and yref.shape == (G * gsz, N + 1, 6)
    for world in (2, 5):
        xs, ys = [], []
        for r in range(world):
            g_lo, g_hi, _, _ = shard_groups(G, gsz, world, r)
            a, b, _ = config_groups(cid, g_lo, g_hi, G, N=N)
            xs.append(a); ys.append(b)
        assert np.array_equal(np.vstack(xs), x0) and np.array_equal(np.vstack(ys), yref)
    if gsz > 1:
        yg = yref.reshape(G, gsz, N + 1, 6)
        assert (yg == yg[:, :1]).all()
        d = x0.reshape(G, gsz, 8)[:, 1:] - x0.reshape(G, gsz, 8)[:, :1]
        stds = np.asarray(config.MPC["stds"])
        assert (d[:, :, stds == 0] == 0).all()
        if cid == 3:        # the same 15 sigma points for every pose
            assert np.allclose(d, d[:1], atol=1e-12)
        else:               # i.i.d. draws: different per pose, sample std near the configured one
            assert not np.allclose(d[0], d[1])
            sd = d[:, :, stds > 0].reshape(-1, 3).std(axis=0)
            assert np.all(np.abs(sd / stds[stds > 0] - 1) < 0.25)


def _gloo_group_worker(rank, world, port, out):
    import torch
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    from tum_control_amd.sharding import ResultGatherer, shard_groups
    from tum_control_amd.workloads import config_groups
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    G, gsz, N = 6, 16, 6
    g_lo, g_hi, b_lo, b_hi = shard_groups(G, gsz, world, rank)
    x0, yref, _ = config_groups(4, g_lo, g_hi, G, N=N)
    # stand-in for the result slab of bench.py: 5 doubles per instance (first = the instance's global index, then x0[3:7])
    # followed by one 16-double record per group (its index and the group mean of x0): ONE flat buffer, ONE gather
    per = np.concatenate([np.arange(b_lo, b_hi)[:, None].astype(float), x0[:, 3:7]], axis=1)
    grp = np.concatenate([np.arange(g_lo, g_hi)[:, None].astype(float), x0.reshape(-1, gsz, 8).mean(axis=1), np.zeros((g_hi - g_lo, 7))], axis=1)
    slab = torch.from_numpy(np.concatenate([per.reshape(-1), grp.reshape(-1)])).reshape(1, -1)
    g = ResultGatherer(world, rank, 1, torch.device("cpu"), nf=slab.shape[1], ni=1)
    af, _ = g.gather(slab)
    if rank == 0:
        out.put(af.numpy().copy())
    dist.barrier()
    dist.destroy_process_group()


def test_group_sharded_gather_world2_gloo():
    """N > 1 path of bench.py --config 3/4 on CPU: two processes (gloo), group-aligned shards of the Monte-Carlo workload,
    one rooted gather of the flat slab (per-instance part + per-group part); the root reassembles the unsharded job."""
    import torch.multiprocessing as mp
    from tum_control_amd.workloads import config_groups
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000)
    ps = [ctx.Process(target=_gloo_group_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    af = q.get(timeout=180)
    for p in ps:
        p.join(timeout=120)
        assert p.exitcode == 0
    G, gsz, N = 6, 16, 6
    x0, _, _ = config_groups(4, 0, G, G, N=N)
    nper = (G // 2) * gsz
    per = np.vstack([af[r, 0, :nper * 5].reshape(nper, 5) for r in range(2)])
    grp = np.vstack([af[r, 0, nper * 5:].reshape(G // 2, 16) for r in range(2)])
    assert np.array_equal(per[:, 0], np.arange(G * gsz)) and np.array_equal(per[:, 1:], x0[:, 3:7])
    assert np.array_equal(grp[:, 0], np.arange(G))
    np.testing.assert_allclose(grp[:, 1:9], x0.reshape(G, gsz, 8).mean(axis=1), atol=1e-13)
    # rank boundaries fall on group boundaries
    assert nper % gsz == 0


def _gloo_worker(rank, world, port, out):
    import torch
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    from tum_control_amd.sharding import ResultGatherer, shard_range
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    per = 5
    lo, hi = shard_range(world * per, world, rank)
    f = torch.arange(lo, hi, dtype=torch.float64).reshape(-1, 1).repeat(1, 3) + torch.tensor([0.0, 0.25, 0.5], dtype=torch.float64)
    i = torch.stack([torch.arange(lo, hi, dtype=torch.int32), torch.full((per,), rank, dtype=torch.int32)], 1)
    g = ResultGatherer(world, rank, per, torch.device("cpu"))
    for _ in range(2):      # buffers are reused across steps
        af, ai = g.gather(f, i)
    if rank == 0:
        out.put((af.reshape(-1, 3).numpy().copy(), ai.reshape(-1, 2).numpy().copy()))
    dist.barrier()
    dist.destroy_process_group()


def test_result_gather_world2_gloo():
    """N > 1 path on CPU: two processes, gloo, rooted gather of the result slabs in shard order."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000)
    ps = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    af, ai = q.get(timeout=120)
    for p in ps:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert np.array_equal(af[:, 0], np.arange(10.0)) and np.allclose(af[:, 2] - af[:, 0], 0.5)
    assert np.array_equal(ai[:, 0], np.arange(10)) and np.array_equal(ai[:, 1], np.repeat([0, 1], 5))


def test_cabi_exports_every_declared_symbol():
    """The built .so loads and exports every function include/tum_nmpc.h declares."""
    import __graft_entry__ as g
    g.build()
    from tum_control_amd import solver
    hdr = open(os.path.join(ROOT, "include", "tum_nmpc.h")).read()
    declared = sorted(set(re.findall(r"\b(tum_(?:ocp|pce|sim|planner)_\w+)\s*\(", hdr)))
    assert len(declared) >= 20
    L = solver.load_library()
    for sym in declared:
        assert hasattr(L, sym), sym
    assert sorted(solver.C_SYMBOLS) == declared


def test_shipped_kernels_resource_budget():
    """What the compiler reports for every kernel of the SHIPPED library (build() keeps the kernel-resource-usage remarks in
    libtumnmpc.so.resources): no kernel spills more than 64 SGPRs (the fused kernel's 129-158 went with an unexplained
    miscompile, HISTORY.md (round-4 document, section 7) -- it lives in the development build only), scratch stays small everywhere, and the headline
    instantiation of the interior point kernel has no spills, no scratch and one wavefront per SIMD."""
    import shutil
    import subprocess
    import __graft_entry__ as g
    if not (os.path.exists(g.HIPCC) or shutil.which("hipcc")) and not os.path.exists(g.LIB + ".resources"):
        pytest.skip("no hipcc and no resource table of a previous build on this host")
    g.build()
    rows = {}
    for line in open(g.LIB + ".resources"):
        parts = line.split()
        rows[parts[0]] = [int(x) for x in parts[1:]]
    assert len(rows) >= 20
    # kernels are looked up by their demangled names (the mangling is the compiler's business)
    filt = shutil.which("c++filt") or "/opt/rocm/lib/llvm/bin/llvm-cxxfilt"
    names = list(rows)
    dem = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    rows = {d.strip(): rows[n] for n, d in zip(names, dem)}

    def kernel(sub):
        hit = [v for n, v in rows.items() if sub in n]
        assert len(hit) == 1, (sub, [n for n in rows if sub in n])
        return hit[0]
    assert not any("nmpc_rti_kernel" in n or "ipm4_kernel" in n for n in rows), "development kernels in the shipped library"
    for name, (vgpr, agpr, sgpr_spill, vgpr_spill, scratch, lds, occ) in rows.items():
        assert sgpr_spill <= 64, (name, sgpr_spill)
        # no scratch anywhere: the condensing kernel's 52 B of rounds 2-3 are gone, and since round 6 (lane-distributed micro-panels: ~26
        # registers fewer) the six-tile interior point kernel (N = 41..48) no longer spills its 10 registers / 44 B either
        # -- the five- and six-tile builds. The seven-tile interior point kernel (N = 49..56, round 6: 112 registers of gg rows alone) spills: stated
        # in INTEGRATION.md with its measured rate
        if "ipm_kernel<false, 7" in name:
            assert scratch <= 256 and vgpr_spill <= 64, (name, scratch, vgpr_spill)
        else:
            assert scratch == 0 and vgpr_spill == 0, (name, scratch, vgpr_spill)
        # (cond_wide_kernel: one workgroup of six wavefronts per CU by design -- records, row store of every stage and g column in LDS)
        lds_cap = 160 * 1024 if "cond_wide_kernel" in name else 40 * 1024
        assert vgpr + agpr <= 512 and lds <= lds_cap, name
    for name in ("ipm_kernel<false, 5, true>", "ipm_kernel<false, 5, false>", "ipm_kernel<false, 6, true>", "ipm_kernel<false, 6, false>"):      # headline: the expansion fused into its tail; SNMPC: without; the six-tile build
        ipm = kernel(name)
        assert ipm[2:5] == [0, 0, 0] and ipm[6] == 1, (name, ipm)
    cond = kernel("cond_kernel<5, false, true>")            # the headline's: the register form of the stage record
    assert cond[2:5] == [0, 0, 0] and cond[6] == 2          # no spills, two wavefronts per SIMD


def test_no_cpu_fallback():
    """Without a GPU the product must fail loudly, never compute on the CPU."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from tum_control_amd.solver import BatchedOcpSolver
    with pytest.raises(RuntimeError, match="no HIP device|failed"):
        BatchedOcpSolver(N=38, batch=1)


def test_product_never_imports_oracle():
    pk = os.path.join(ROOT, "tum-control_amd")
    for dp, _, fs in os.walk(pk):
        for f in fs:
            if f.endswith((".py", ".hip", ".hpp", ".h", ".cpp")):
                txt = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", txt, re.M), f
                assert "liboracle" not in txt and "oracle/" not in txt, f


def test_pce_helpers_match_reference_golden(golden_dir):
    """alphaGeneration / hermiteGeneration / polyChaosExpansion / compute_x0dist restatements vs values captured
    from the reference, and the Hammersley recipe vs the sigma points stored in acados_ocp_SNMPC.json."""
    from tum_control_amd import snmpc
    g = np.load(os.path.join(golden_dir, "pce.npz"))
    assert np.array_equal(snmpc.alpha_generation(3, 2), g["alphas"])
    for i, x in enumerate((-1.3, 0.0, 0.4, 2.2)):
        for n in range(4):
            assert abs(snmpc.hermite(x, n) - g["herm"][i, n]) < 1e-14
    for i in range(g["w"].shape[1]):
        np.testing.assert_allclose(snmpc.pce_basis(g["w"][:, i], g["alphas"]), g["phi"][i], atol=1e-13)
    np.testing.assert_allclose(snmpc.compute_x0dist(g["x0"], g["w"], g["stds"]), g["x0dist"], atol=1e-14)
    # sigma points of the exported SNMPC OCP: n_s = 10, stds at export time (1.1, 0.2, 0.05) on states 3,4,5
    w = snmpc.hammersley_normal(10, 3)
    lb = g["json_lbx0"]
    off = snmpc.x0_offsets(w, [0, 0, 0, 1.1, 0.2, 0.05, 0, 0])
    np.testing.assert_allclose(lb[1:] - lb[0], off, atol=1e-12)
    A = snmpc.pce_matrix(w, snmpc.alpha_generation(3, 2))
    assert A.shape == (10, 10)
    # the PCE of a constant is that constant with zero variance
    c = A @ np.full(10, 3.5)
    assert abs(c[0] - 3.5) < 1e-9 and np.abs(c[1:]).max() < 1e-9


def test_r2_setup_matches_reference_propagation(golden_dir):
    from tum_control_amd.r2nmpc import r2_setup
    g = np.load(os.path.join(golden_dir, "r2.npz"))
    # P_propagation golden: A P A' + B W B'
    for i in range(len(g["P"])):
        np.testing.assert_allclose(g["A"][i] @ g["P"][i] @ g["A"][i].T + g["B"][i] @ g["W"] @ g["B"][i].T, g["Pn"][i], atol=1e-10)
    S0, BWB = r2_setup([0, 0, 0, 0.8, 0.35, 0.035, 0, 0], 0.08)
    assert S0.shape == (8, 8) and abs(S0[3, 3] - (0.5 * 0.8) ** 2) < 1e-15 and abs(S0[0, 0] - (0.5e-5) ** 2) < 1e-20
    assert abs(BWB[4, 4] - 0.08 * 0.35 ** 2) < 1e-15 and BWB[6, 6] == 0.0 and BWB[2, 2] == 0.0


def test_plant_restatement_reproduces_logged_closed_loops(golden_dir):
    """7-state plant + RK4 x 4 over Ts = 0.02 s (Vehicle_Simulator/...): CiLX[i+1] from (CiLX[i], a = MPC_SimX[i+1][7],
    steering rate = simU[i][1]) for the 26 logged closed loops x 150 steps."""
    from tum_control_amd.closed_loop import plant_step, MovingAverageEstimator
    from tum_control_amd import config
    d = np.load(os.path.join(golden_dir, "closed_loop_monteblanco_150.npz"))
    C = d["CiLX"].copy(); C[:, :, 2] = np.unwrap(C[:, :, 2], axis=1)
    cfg = config.default_config()
    for i in range(150):
        xn = plant_step(C[:, i], d["MPC_SimX"][:, i + 1, 7], d["simU"][:, i, 1], cfg)
        assert np.abs(xn - C[:, i + 1]).max() < 1e-12
    # estimator: truncated moving averages with windows [1,1,4,2,2,3,4,2]
    est = MovingAverageEstimator(1)
    xs = np.arange(40.0).reshape(5, 1, 8)
    outs = [est(x)[0] for x in xs]
    assert outs[4][0] == xs[4, 0, 0] and outs[4][2] == xs[1:5, 0, 2].mean() and outs[1][6] == xs[:2, 0, 6].mean()


# ------------------------------------------------------------------------------------------------ bench.py, N > 1 control flow
class _StandInSolver:
    """CPU stand-in with the methods bench.py calls on BatchedOcpSolver: "solving" instance b yields
    u0 = 2 x0[3:5], cost = sum(x0), status 0, qp_iter 5 + (b mod 3); device pointers are host pointers here."""

    def __init__(self, N, dt, nsub, batch, device=0, store_qp_in=False):
        from tum_control_amd import config
        self.N, self.B = N, batch
        self.cfg = config.default_config()
        self.x0 = np.zeros((batch, 8)); self.yref = np.zeros((batch, N + 1, 6))
        self.res = np.zeros((batch, 5)); self.calls = dict(cold=0, solve=0, put=0, summary=0)

    @staticmethod
    def _view(ptr, n):
        import ctypes
        return np.ctypeslib.as_array((ctypes.c_double * n).from_address(ptr))

    def install_reference_ocp(self): pass
    def set_x0(self, x0): self.x0[:] = x0
    def set_yref_all(self, y): self.yref[:] = y
    def set_schedule(self, on): pass
    def cold_start(self): self.calls["cold"] += 1

    def put_device(self, field, ptr):
        self.calls["put"] += 1
        if field == "x0":
            self.x0[:] = self._view(ptr, self.B * 8).reshape(self.B, 8)
        else:
            self.yref[:] = self._view(ptr, self.yref.size).reshape(self.yref.shape)

    def solve_async(self):
        self.calls["solve"] += 1
        self.res[:, 0:2] = 2.0 * self.x0[:, 3:5]; self.res[:, 2] = self.x0.sum(axis=1)
        self.res[:, 3] = 0.0; self.res[:, 4] = 5 + (np.arange(self.B) % 3)

    def get_device(self, field, ptr):
        if field == "X":          # (--gather-iterate) a recognisable iterate: X[b, k, i] = x0[b, i] + k, U[b, k, j] = res[b, j] - k
            self._view(ptr, self.B * (self.N + 1) * 8)[:] = (self.x0[:, None, :] + np.arange(self.N + 1)[None, :, None]).reshape(-1)
            return
        if field == "U":
            self._view(ptr, self.B * self.N * 2)[:] = (self.res[:, None, :2] - np.arange(self.N)[None, :, None]).reshape(-1)
            return
        assert field == "summary"
        self.calls["summary"] += 1
        self._view(ptr, self.B * 5)[:] = self.res.reshape(-1)

    def get_stats(self, f):
        return self.res[:, 3].astype(int) if f == "status" else self.res[:, 4].astype(int)

    def get_cost(self):
        return self.res[:, 2].copy()

    def get_iterate(self):
        return None, np.zeros((self.B, self.N, 2))


def _gloo_bench_worker(rank, world, port, out, argv):
    import torch
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    import bench
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    args = bench.parse_args(argv)
    assert dist.get_world_size() == args.gpus
    res = bench.run(args, torch, dist, torch.device("cpu"), world, rank, rank, _StandInSolver)
    if rank == 0:
        o, job = res
        calls = {k: sum(sv.calls[k] for sv in job.ring) for k in job.s.calls}
        out.put((o, job.gather.all_f.numpy().copy(), calls, job.slab_pad, job.B, [dict(sv.calls) for sv in job.ring]))
    else:
        assert res is None
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("scaling", ["weak", "strong", "weak+iterate"])
def test_bench_control_flow_world2_gloo(scaling):
    """bench.py's own step / gather / timing control flow at world size 2 on CPU (gloo), with a stand-in solver: what the
    driver's first real multi-GPU run executes, minus the kernels. Weak scaling: every rank its share; strong scaling: a fixed
    global batch of 5 scenario groups cut 3 + 2 (unequal shards: the gathered slab is padded to the largest)."""
    import json
    import torch.multiprocessing as mp
    from tum_control_amd.workloads import config_groups
    steps, warm, N = 3, 1, 6
    with_iterate = scaling.endswith("+iterate")          # (--gather-iterate: X and U ride behind the summary in the same rooted gather)
    scaling = scaling.split("+")[0]
    argv = ["--gpus", "2", "--steps", str(steps), "--warmup", str(warm), "--config", "4", "--horizon", str(N), "--no-cpu-baseline",
            "--streams", "2"] + (["--gather-iterate"] if with_iterate else [])
    argv += ["--batch", "48"] if scaling == "weak" else ["--scaling", "strong", "--global-batch", "80"]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33500 + (os.getpid() % 2000) + (7 if scaling == "strong" else 0) + (13 if with_iterate else 0)
    ps = [ctx.Process(target=_gloo_bench_worker, args=(r, 2, port, q, argv)) for r in range(2)]
    for p in ps:
        p.start()
    o, allf, calls, pad, B0, per_slot = q.get(timeout=240)
    for p in ps:
        p.join(timeout=120)
        assert p.exitcode == 0
    G = 6 if scaling == "weak" else 5
    sizes = [48, 48] if scaling == "weak" else [48, 32]
    json.dumps(o)                                        # the line must serialise
    assert o["n_gpus"] == 2 and o["scaling"] == scaling and o["steps"] == steps
    assert o["config"]["global_batch"] == 16 * G and o["config"]["batch_per_gpu"] == sizes[0] == B0
    assert o["value"] > 0 and abs(o["value"] * o["ms_per_step"] * 1e-3 - 16 * G) < 1e-6 * 16 * G
    assert o["solve_ms_per_step"] >= 0 and o["gather_ms_per_step"] >= 0
    assert o["status_ok_frac"] == 1.0
    # every step: one cold start, one solve, one summary pack, one rotation of the inputs (x0 + yref), dealt to the two
    # capsules of the ring in turn
    n = steps + warm
    assert calls == dict(cold=n, solve=n, put=2 * n, summary=n) and o["config"]["streams"] == 2
    assert [c["solve"] for c in per_slot] == [n - n // 2, n // 2]
    # what the root holds after the last step = the stand-in's results for the last rotated batch, in shard order
    per_inst = 5 + (((N + 1) * 8 + N * 2) if with_iterate else 0)
    assert pad == 48 * per_inst and allf.shape == (2, 1, pad) and o["config"]["gather_iterate"] == with_iterate
    assert o["config"]["gather_bytes_per_rank"] == 8 * pad
    variant = (steps - 1) % 4 + 1
    x0, _, _ = config_groups(4, 0, G, G, N=N, variant=variant)
    lo = 0
    for r, sz in enumerate(sizes):
        got = allf[r, 0, :sz * 5].reshape(sz, 5)
        np.testing.assert_array_equal(got[:, 0:2], 2.0 * x0[lo:lo + sz, 3:5])
        np.testing.assert_allclose(got[:, 2], x0[lo:lo + sz].sum(axis=1), rtol=1e-15)
        assert (got[:, 3] == 0).all() and np.array_equal(got[:, 4], 5 + (np.arange(sz) % 3))
        if with_iterate:          # X and U of the rank's shard behind the summary block (blocks sized for the largest shard: 48)
            X = allf[r, 0, 48 * 5:48 * 5 + sz * (N + 1) * 8].reshape(sz, N + 1, 8)
            U = allf[r, 0, 48 * 5 + 48 * (N + 1) * 8:48 * 5 + 48 * (N + 1) * 8 + sz * N * 2].reshape(sz, N, 2)
            np.testing.assert_array_equal(X, x0[lo:lo + sz, None, :] + np.arange(N + 1)[None, :, None])
            np.testing.assert_array_equal(U, got[:, None, :2] - np.arange(N)[None, :, None])
        lo += sz


def test_bench_launches_its_own_ranks_world2_gloo(tmp_path):
    """`python bench.py --gpus 2` with NO launcher around it (the shape of the driver's BENCH command with a larger N): bench.py
    starts its two ranks itself (bench.self_launch: RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR = 127.0.0.1 / a free port, as
    torch.distributed.run sets them), the ranks form a process group (gloo here, with the stand-in solver the test supplies through
    TUM_BENCH_TEST_SOLVER; nccl = RCCL on GPUs), rank 0 prints the ONE JSON line, exit code 0. Round 5's bench.py exited with
    "launch with torch.distributed.run" here. --dump-outputs: rank 0 writes its capsule's results and the summary of all 96 instances as the
    rooted gather delivered it."""
    import json
    import subprocess
    env = dict(os.environ, TUM_BENCH_TEST_SOLVER="test_host_logic:_StandInSolver",
               PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "tests"), ROOT, os.environ.get("PYTHONPATH", "")]))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "BENCH_SELF_LAUNCHED"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--config", "4", "--horizon", "6",
           "--batch", "48", "--streams", "2", "--no-cpu-baseline", "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    assert len(lines) == 1, r.stdout[-2000:]
    o = json.loads(lines[0])
    assert o["n_gpus"] == 2 and o["steps"] == 3 and o["scaling"] == "weak"
    assert o["launch"].startswith("self-launched")
    assert o["config"]["collective_backend"] == "gloo" and o["config"]["collective_world_size"] == 2
    assert o["config"]["global_batch"] == 96 and o["config"]["batch_per_gpu"] == 48
    assert o["value"] > 0 and abs(o["value"] * o["ms_per_step"] * 1e-3 - 96) < 1e-6 * 96
    assert len(o["per_rank"]["value"]) == 2 and all(v > 0 for v in o["per_rank"]["value"])
    assert o["value"] <= sum(o["per_rank"]["value"]) * (1 + 1e-9)          # the job's rate is set by the slowest rank
    assert o["gather_ms_per_step"] >= 0 and o["status_ok_frac"] == 1.0
    assert "stand-in" in o["data"] and o["cpu_baseline"] is None
    g = np.load(tmp_path / "gathered_summary.npy")
    assert g.shape == (96, 5) and g.dtype == np.float64
    from tum_control_amd.workloads import config_groups
    x0, _, _ = config_groups(4, 0, 6, 6, N=6, variant=3)          # the last timed step's batch, both shards in rank order
    np.testing.assert_allclose(g[:, 2], x0.sum(axis=1), rtol=1e-15)
    np.testing.assert_array_equal(g[:, 4], 5 + (np.tile(np.arange(48), 2) % 3))
    np.testing.assert_array_equal(g[:48, 2], np.load(tmp_path / "cost.npy"))


def test_bench_self_launch_propagates_a_failing_rank():
    """a rank that dies takes the job down with a non-zero exit code and no JSON line (here: more ranks than scenario groups)"""
    import subprocess
    env = dict(os.environ, TUM_BENCH_TEST_SOLVER="test_host_logic:_StandInSolver",
               PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "tests"), ROOT, os.environ.get("PYTHONPATH", "")]))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "BENCH_SELF_LAUNCHED"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--config", "4", "--horizon", "6",
           "--scaling", "strong", "--global-batch", "16", "--no-cpu-baseline"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert not [ln for ln in r.stdout.splitlines() if '"metric"' in ln]


def test_bench_plain_run_and_its_outputs(tmp_path):
    """`python bench.py --gpus 1` without --full (stand-in solver on CPU): exactly --steps timed steps, none of the --full legs in the line;
    --dump-outputs writes what the last timed step computed as float64 .npy files, the same ones for the same arguments. Beyond the size
    limit every array keeps the same seeded sample of its rows."""
    import json
    import subprocess
    import bench
    from tum_control_amd.workloads import config_groups
    env = dict(os.environ, TUM_BENCH_TEST_SOLVER="test_host_logic:_StandInSolver",
               PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "tests"), ROOT, os.environ.get("PYTHONPATH", "")]))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "BENCH_SELF_LAUNCH", "BENCH_SELF_LAUNCHED"):
        env.pop(k, None)
    dumps = []
    for run in range(2):
        d = tmp_path / f"out{run}"
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--config", "4", "--horizon", "6",
               "--batch", "48", "--streams", "2", "--dump-outputs", str(d)]
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
        assert len(lines) == 1, r.stdout[-2000:]
        o = json.loads(lines[0])
        assert o["steps"] == 3 and o["full"] is False and o["launch"] == "single process"
        assert o["value"] > 0 and abs(o["value"] * o["ms_per_step"] * 1e-3 - 48) < 1e-6 * 48
        for k in ("other_configs", "n38", "cpu_baseline", "parity_vs_oracle_max_abs_u0"):
            assert k not in o, k
        assert o["value_single_stream"] is None and o["value_host_visible"] is None and o["value_repeated_batch"] is None
        assert o["roofline"]["dominant"] is None
        got = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
        assert sorted(got) == ["U", "cost", "qp_iter", "status"] and all(a.dtype == np.float64 for a in got.values())
        dumps.append(got)
    for k in dumps[0]:
        np.testing.assert_array_equal(dumps[0][k], dumps[1][k])
    # the last timed step solved fresh batch 3 (variant (steps - 1) mod nb + 1) on capsule 1 (four steps over two capsules)
    x0, _, _ = config_groups(4, 0, 3, 3, N=6, variant=3)
    np.testing.assert_allclose(dumps[0]["cost"], x0.sum(axis=1), rtol=1e-15)
    np.testing.assert_array_equal(dumps[0]["qp_iter"], 5 + (np.arange(48) % 3))
    # the size limit: 1000 x (8 + 1) doubles + 1000 x 2 doubles + index files > 40 kB
    arrays = {"a": np.arange(8000.0).reshape(1000, 8), "b": np.arange(1000.0), "c": np.arange(2000.0).reshape(1000, 2)}
    for run in range(2):
        bench.write_outputs(str(tmp_path / f"cut{run}"), arrays, limit=40000)
    files = sorted(os.listdir(tmp_path / "cut0"))
    assert files == ["a.npy", "a_rows.npy", "b.npy", "b_rows.npy", "c.npy", "c_rows.npy"]
    assert sum(os.path.getsize(tmp_path / "cut0" / f) for f in files) <= 40000
    rows = np.load(tmp_path / "cut0" / "a_rows.npy")
    assert 0 < len(rows) < 1000 and (np.diff(rows) > 0).all()
    for name in ("a", "b", "c"):
        np.testing.assert_array_equal(np.load(tmp_path / "cut0" / f"{name}_rows.npy"), rows)
        np.testing.assert_array_equal(np.load(tmp_path / "cut0" / f"{name}.npy"), arrays[name][rows.astype(int)])
        np.testing.assert_array_equal(np.load(tmp_path / "cut0" / f"{name}.npy"), np.load(tmp_path / "cut1" / f"{name}.npy"))

def test_workload_variants_are_fresh_batches_of_the_same_workload():
    """variant 0 is the BASELINE configuration; variants k > 0 (what bench.py rotates through) differ from it and from each
    other in every instance but keep the group structure (one yref per scenario group)."""
    from tum_control_amd.workloads import config_groups
    for cid, G in ((2, 8), (3, 4), (4, 4), (5, 8)):
        b = [config_groups(cid, 0, G, G, N=6, variant=k) for k in range(3)]
        ref = config_groups(cid, 0, G, G, N=6)
        assert np.array_equal(b[0][0], ref[0]) and np.array_equal(b[0][1], ref[1])
        gsz = b[0][2]
        for k in (1, 2):
            assert b[k][0].shape == b[0][0].shape and not np.array_equal(b[k][0][:, :2], b[0][0][:, :2])
            y = b[k][1].reshape(G, gsz, 7, 6)
            assert (y == y[:, :1]).all()
        assert not np.array_equal(b[1][0], b[2][0])


def test_solver_ring_results_bookkeeping():
    """streaming.SolverRing: capsules handed out in turn; up to two result requests are remembered per slot and taken oldest
    first, `drain` walks the outstanding ones in the order the batches were enqueued (host logic only: stand-in capsules)."""
    from tum_control_amd.streaming import SolverRing

    class Fake:
        def __init__(self, i):
            self.i, self.calls, self.n_req, self.n_wait = i, [], 0, 0

        def results_async(self, with_iterate):
            self.calls.append(("async", with_iterate)); self.n_req += 1

        def results_wait(self):
            self.n_wait += 1
            return ("summary", self.i, self.n_wait), None, None

    ring = SolverRing(3, Fake)
    assert [ring.acquire()[0] for _ in range(4)] == [0, 1, 2, 0]          # next turn: capsule 1
    assert ring.take_results(1) is None and list(ring.drain()) == []
    ring.request_results(2, with_iterate=True); ring.request_results(0); ring.request_results(1); ring.request_results(2)
    assert ring[2].calls == [("async", True), ("async", False)] and ring[0].calls == [("async", False)]
    assert [ring.outstanding(i) for i in range(3)] == [1, 1, 2]
    assert ring.take_results(2)[0] == ("summary", 2, 1) and ring.outstanding(2) == 1
    ring.request_results(2)
    # drain: capsule 2 holds an older batch (two outstanding) -> first; then from the capsule whose turn is next
    assert [(i, r[0][2]) for i, r in ring.drain()] == [(2, 2), (1, 1), (2, 3), (0, 1)]
    assert list(ring.drain()) == [] and ring.take_results(2) is None
    with pytest.raises(ValueError):
        SolverRing(0, Fake)
    # more capsules than hardware queues: measured slower on the MI355X (streams share queues) -> refused unless the caller insists
    from tum_control_amd import streaming
    with pytest.raises(ValueError, match="allow_unstable"):
        SolverRing(5, Fake, streams=None)
    assert streaming.MAX_STABLE_SLOTS == 4 and ring.n_slots == len(ring) == 3
    assert len(SolverRing(5, Fake, allow_unstable=True)) == 5


def test_external_cost_type_is_refused_loudly(monkeypatch):
    """NMPC_class.py:90-94 builds a different OCP for costfunction_type != 'NONLINEAR_LS' (the EXTERNAL-cost development
    variant): the mirrors refuse that configuration before anything touches the GPU instead of solving the NONLINEAR_LS problem
    under another name."""
    from tum_control_amd import config, nmpc, snmpc
    cfg = config.default_config(); cfg["mpc"]["costfunction_type"] = "EXTERNAL"
    monkeypatch.setattr(nmpc._config, "default_config", lambda: cfg)
    monkeypatch.setattr(snmpc._config, "default_config", lambda: cfg)
    sim = dict(Tp=3.04, Ts=0.02, Ts_MPC=0.08)
    for C in (nmpc.Nonlinear_Model_Predictive_Controller, snmpc.Stochastic_Nonlinear_Model_Predictive_Controller):
        with pytest.raises(NotImplementedError, match="EXTERNAL"):
            C(sim_main_params=sim, X0_MPC=np.zeros(8))
    from tum_control_amd.r2nmpc import Reduced_Robustified_Nonlinear_Model_Predictive_Controller as R2
    with pytest.raises(NotImplementedError, match="EXTERNAL"):
        R2(sim_main_params=sim, X0_MPC=np.zeros(8))
    nmpc.check_costfunction_type({"costfunction_type": "NONLINEAR_LS"}); nmpc.check_costfunction_type({})


def test_disturbance_generators_match_the_reference(golden_dir):
    """closed_loop.generate_disturbances / DisturbanceModel / lon_lat_deviations / wrap_yaw against what the reference's own functions
    returned (tests/golden/make_golden.py::make_disturbances: Utils/MPC_sim_utils.py:15-134 imported, numpy's global generator seeded)."""
    from tum_control_amd import closed_loop as cl
    d = np.load(os.path.join(golden_dir, "disturbances.npz"))
    m = cl.DisturbanceModel(simulate_disturbances=True, simulate_state_estimation=True)
    np.testing.assert_array_equal(np.array(m.bounds_derivatives), d["bounds_derivatives"])
    np.testing.assert_array_equal(np.array(m.bounds_state_estimation), d["bounds_state_estimation"])
    assert m.types == list(d["types"])
    for kind in ("uniform", "gaussian", "absolute", "box"):
        for name, bounds, seed in (("deriv", m.bounds_derivatives, 7), ("est", m.bounds_state_estimation, 8)):
            rng = np.random.RandomState(seed)
            got = np.array([cl.generate_disturbances(bounds, kind, rng) for _ in range(5)])
            np.testing.assert_allclose(got, d[f"{name}_{kind}"], rtol=1e-14, atol=0)
    w, e = m.draw(6, batch=2, seed=3)          # vehicle 0 of a batch = the reference's run after np.random.seed(3)
    np.testing.assert_allclose(w[:, 0], d["run_w"], rtol=1e-14); np.testing.assert_allclose(e[:, 0], d["run_e"], rtol=1e-14)
    assert not np.array_equal(w[:, 1], w[:, 0])
    yaw, ex, ey, rx, ry = d["dev_in"]
    dl, dt_ = cl.lon_lat_deviations(yaw, ex, ey, rx, ry)
    np.testing.assert_array_equal(dl, d["dev_long"]); np.testing.assert_array_equal(dt_, d["dev_lat"])
    np.testing.assert_array_equal(cl.wrap_yaw(yaw), d["wrapped"])


def test_log_file_has_the_reference_schema(tmp_path, golden_dir):
    """closed_loop.log_file_arrays writes what Logger.save_logs writes (Utils/Logging_Plotting.py:357-372): every key a reader of the
    reference's full_logs.npz / _baseline/F/<track>/<k>.npz finds, with the reference's shapes and derived channels -- checked on a logged
    acados loop (tests/golden/log_file_lvms_3.npz, the reference's file of loop 3 on LVMS): rebuilt from its five raw logs, the derived
    arrays must equal the ones the reference stored in the same file."""
    from tum_control_amd import closed_loop as cl
    r = np.load(os.path.join(golden_dir, "log_file_lvms_3.npz"))
    assert set(cl.LOG_KEYS) == set(r.files)
    # a batch of one vehicle; the file holds 5499 of the 5500 steps that were run (Logger.truncate): give the last one back as a copy
    raw = {k: r[k][:, None] for k in ("CiLX", "MPC_SimX", "simU", "simREF", "simSolverDebug")}
    for k in ("simU", "simREF", "simSolverDebug"):
        raw[k] = np.concatenate([raw[k], raw[k][-1:]])
    for k in ("CiLX", "MPC_SimX"):
        raw[k] = np.concatenate([raw[k], raw[k][-1:]])
    a = cl.log_file_arrays(raw, 0, T=110.0)
    assert cl.log_file_arrays(raw, 0)["t"][-1] == 100.0          # default: sim_main_params['T'] as Logger.save_logs takes it, not the run length
    p = tmp_path / "full_logs.npz"
    np.savez(p, **a)
    mine = np.load(p)
    assert set(mine.files) == set(r.files)
    for k in r.files:
        assert mine[k].shape == r[k].shape, k
        np.testing.assert_allclose(mine[k], r[k], rtol=1e-12, atol=1e-12, err_msg=k)


def test_dpp_operands_of_the_condensing_kernel_are_settled(tmp_path):
    """(Round 6: the interior point kernel's lane-distributed micro-panels use the same instruction -- fnmac_bc / mul_bc_fresh of csrc/pipe_kernels.hpp --
    and are covered by the same scan, plus the check of their results' consumers among the matrix instructions.)
    cond_kernel reads its stage record with `v_fmac_f64_dpp ... row_newbcast:n` written as inline asm (csrc/pipe_kernels.hpp,
    RecRows): the compiler's hazard recogniser does not look into it, and gfx9 needs two wait states between a vector instruction
    that WRITES a register and a DPP read of it (five after one that writes EXEC). The record registers are only ever written by
    loads -- unless the register allocator copies them. This test disassembles the shipped library and checks every DPP accumulation:
    no vector instruction in the two issue slots in front of it (an `s_nop n` counts n + 1) writes its DPP source, none in the five
    in front of it writes EXEC."""
    import re
    import shutil
    import subprocess
    import __graft_entry__ as g
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump) or not os.path.exists(g.LIB):
        pytest.skip("no llvm-objdump / no built library on this host")
    lib = shutil.copy(g.LIB, tmp_path / "lib.so")
    subprocess.run([objdump, "--offloading", str(lib)], cwd=tmp_path, check=True, capture_output=True)
    co = [f for f in os.listdir(tmp_path) if "gfx950" in f]
    assert len(co) == 1, os.listdir(tmp_path)
    dis = subprocess.run([objdump, "-d", "--no-show-raw-insn", str(tmp_path / co[0])], capture_output=True, text=True, check=True).stdout

    def regs(tok):
        m = re.fullmatch(r"v\[(\d+):(\d+)\]", tok)
        if m:
            return set(range(int(m.group(1)), int(m.group(2)) + 1))
        m = re.fullmatch(r"v(\d+)", tok)
        return {int(m.group(1))} if m else set()

    n_dpp = 0
    exec_age = 99        # wait states since a VECTOR instruction wrote EXEC (v_cmpx ...: a DPP operation needs five behind it)
    window = []          # (registers written by a vector instruction, wait states it is away from the next instruction)
    dpp_window = []      # the same for the DPP accumulations alone (their consumers among the matrix instructions)
    for line in dis.splitlines():
        s = line.split("//")[0].strip()
        if not s or s.endswith(":") or not re.match(r"^[a-z]", s):
            continue
        op, _, rest = s.partition(" ")
        ops = [t.strip() for t in rest.split(",")] if rest else []
        if op.startswith("v_fmac_f64_dpp"):
            n_dpp += 1
            src = regs(ops[1].split()[0].lstrip("-"))          # (a negated broadcast operand: -v[a:b])
            assert src, s
            for written, dist in window:
                assert dist >= 2 or not (written & src), ("a vector instruction writes the DPP source within two wait states", s)
            assert exec_age >= 5, ("a vector instruction writes EXEC within five wait states of a DPP operation", s)
        if op.startswith("v_mfma"):
            # (round 6, found at N = 48) the hazard recogniser does not know that the inline asm is a vector instruction either: a matrix
            # instruction must not take a register a DPP accumulation wrote within two wait states as its A / B operand
            srcs = set().union(*(regs(t.split()[0]) for t in ops[1:3]))
            for written, dist in dpp_window:
                assert dist >= 2 or not (written & srcs), ("a matrix instruction reads a register a DPP accumulation wrote within two wait states", s)
        ws = (int(ops[0]) + 1) if op == "s_nop" else 1
        dpp_window = [(w, d + ws) for w, d in dpp_window if d + ws < 3]
        if op.startswith("v_fmac_f64_dpp"):
            dpp_window.append((regs(ops[0].split()[0]), 0))
        exec_age = 0 if (op.startswith("v_cmpx") or (op.startswith("v_") and ops and ops[0].split()[0].startswith("exec"))) else min(exec_age + ws, 99)
        window = [(w, d + ws) for w, d in window if d + ws < 3]
        if op.startswith("v_") and not op.startswith(("v_cmp", "v_readlane", "v_readfirstlane")) and ops:
            written = regs(ops[0].split()[0])
            if op.startswith("v_permlane") and len(ops) > 1:
                written |= regs(ops[1].split()[0])
            window.append((written, 0))
    assert n_dpp > 500          # (the register form is in the library: ~110 accumulations per stage instantiation)
