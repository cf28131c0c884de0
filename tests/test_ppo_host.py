"""
The host statements of the PPO update (closed_loop.ppo_loss_and_grads, adam_step, learning_rate_schedule, minibatch_slices) against the
references of tests/ppo_reference.py: the long-double analytic gradients, torch's CPU autograd in float64, torch.optim.Adam. No GPU.
"""
import numpy as np
import pytest

import ppo_reference as ref

CASES = [("odd", 37), ("odd", 200), ("tiny", 17), ("widest", 16), ref.GOLDEN_CASE]


def _policy(name):
    from tum_control_amd.closed_loop import WeightPolicy
    return WeightPolicy(*ref.nets(name))


@pytest.mark.parametrize("name,n", CASES)
def test_host_statement_against_long_double_and_torch(name, n):
    from tum_control_amd.closed_loop import ppo_loss_and_grads
    inp, ld, th = ref.references(name, n)
    # no row near the kink of min(): clip_fraction and the branch of every row are decided
    assert ld["kink"] > 1e-9
    got = ppo_loss_and_grads(_policy(name), inp["obs"], inp["actions"], inp["old_log_probs"], inp["advantages"], inp["returns"], **ref.SETTINGS)
    e_host, e_torch = ref.errors(got["grads"], ld["grads"]), ref.errors(th["grads"], ld["grads"])
    for t, a, b in zip(ref.tensor_names(ld["grads"]), e_host, e_torch):
        print(f"{name} n={n} {t}: host {a:.2f} torch {b:.2f} (units of u max|g|)")
    assert (e_host <= np.maximum(4.0 * e_torch, ref.FLOOR)).all()
    gates = {}
    for k in ref.GATED:
        a, b = ref.scalar_error(got[k], ld[k]), ref.scalar_error(th[k], ld[k])
        print(f"{name} n={n} {k}: host {a:.2f} torch {b:.2f} (units of u |x|)")
        gates[k] = max(4.0 * b, ref.FLOOR)
        assert a <= gates[k], k
    assert abs(ref.LD(got["loss"]) - ld["loss"]) <= ref.loss_bound(ld, gates)
    assert got["clip_fraction"] == ld["clip_fraction"]
    assert 0.5 < ld["unclipped"] < 0.9          # both branches of min() carry rows


def test_one_row_takes_the_advantage_as_it_is():
    from tum_control_amd.closed_loop import ppo_loss_and_grads
    inp = ref.case("odd", 1)
    pol = _policy("odd")
    got = ppo_loss_and_grads(pol, **{k: inp[k] for k in ("obs", "actions", "old_log_probs", "advantages", "returns")}, **ref.SETTINGS)
    ld = ref.loss_and_grads_ld(*ref.nets("odd"), **inp, **ref.SETTINGS, normalize_advantage=False)
    assert np.isfinite(got["loss"]) and abs(ref.LD(got["loss"]) - ld["loss"]) <= ref.loss_bound(ld, dict.fromkeys(ref.GATED, ref.FLOOR))
    assert (ref.errors(got["grads"], ld["grads"]) <= ref.FLOOR).all()


def test_log_probs_and_values_are_the_policys():
    """the statement's forward pass is WeightPolicy's, to the bit: what the collector recorded is what the first epoch's ratio divides by"""
    from tum_control_amd.closed_loop import ppo_loss_and_grads
    inp = ref.case("odd", 37)
    pol = _policy("odd")
    got = ppo_loss_and_grads(pol, inp["obs"], inp["actions"], pol.log_prob(inp["obs"], inp["actions"]), inp["advantages"], inp["returns"])
    assert np.array_equal(got["log_probs"], pol.log_prob(inp["obs"], inp["actions"]))
    assert np.array_equal(got["values"], pol.values(inp["obs"]))
    assert np.array_equal(got["ratio"], np.ones(37)) and got["approx_kl"] == 0.0 and got["clip_fraction"] == 0.0


@pytest.mark.parametrize("max_norm", [0.5, 1e6])
def test_adam_step_against_torch(max_norm):
    """three steps of clip_grad_norm_ + torch.optim.Adam(eps=1e-5) in float64 on the same gradients"""
    import torch
    from tum_control_amd.closed_loop import adam_step
    rng = np.random.RandomState(3)
    shapes = [(7, 5), (7,), (3, 7), (3,)]
    params = [rng.randn(*s) for s in shapes]
    tp = [torch.tensor(p.copy(), requires_grad=True) for p in params]
    opt = torch.optim.Adam(tp, lr=3e-4, eps=1e-5)
    m, v = [np.zeros(s) for s in shapes], [np.zeros(s) for s in shapes]
    for t in (1, 2, 3):
        grads = [rng.randn(*s) * 10.0 ** rng.randint(-3, 1) for s in shapes]
        lr = 3e-4 * t
        for p, g in zip(tp, grads):
            p.grad = torch.tensor(g.copy())
        total_t = float(torch.nn.utils.clip_grad_norm_(tp, max_norm))
        for group in opt.param_groups:
            group["lr"] = lr
        opt.step()
        params, m, v, total = adam_step(params, grads, m, v, t, lr, max_grad_norm=max_norm)
        assert abs(total - total_t) <= 8 * ref.U * total
        assert (total > max_norm) == (max_norm == 0.5)
        for p, q in zip(params, tp):
            q = q.detach().numpy()
            assert np.abs(p - q).max() <= 8 * ref.U * np.abs(q).max()
        for a, q in zip(m, tp):
            assert np.allclose(a, opt.state[q]["exp_avg"].numpy(), rtol=1e-14, atol=0)
        for a, q in zip(v, tp):
            assert np.allclose(a, opt.state[q]["exp_avg_sq"].numpy(), rtol=1e-14, atol=0)


def test_adam_step_against_long_double():
    from tum_control_amd.closed_loop import adam_step
    rng = np.random.RandomState(4)
    params, grads = [rng.randn(40, 3)], [rng.randn(40, 3)]
    m, v = [0.01 * rng.randn(40, 3)], [0.01 * rng.rand(40, 3)]
    P, M, V, total = adam_step(params, grads, m, v, 2, 1e-3, max_grad_norm=0.5)
    Pl, Ml, Vl, tl = ref.adam_ld(params, grads, m, v, 2, 1e-3, 0.5)
    assert abs(total - tl) <= 4 * ref.U * tl
    assert np.abs(P[0] - Pl[0]).max() <= 8 * ref.U * np.abs(Pl[0]).max()
    assert np.abs(M[0] - Ml[0]).max() <= 8 * ref.U * np.abs(Ml[0]).max() and np.abs(V[0] - Vl[0]).max() <= 8 * ref.U * np.abs(Vl[0]).max()


def test_learning_rate_schedule():
    from tum_control_amd.closed_loop import learning_rate_schedule
    f = learning_rate_schedule(3e-4, 1e-5, 2.0)
    for remaining in (1.0, 0.5, 0.0):
        assert f(remaining) == 3e-4 * pow(1e-5 / 3e-4, (1 - remaining) * 2.0)
    assert f(1.0) == 3e-4 and abs(f(0.5) - 1e-5) < 1e-18


def test_minibatch_slices_cut_a_short_last_batch():
    from tum_control_amd.closed_loop import minibatch_slices
    assert [(s.start, s.stop) for s in minibatch_slices(100, 48)] == [(0, 48), (48, 96), (96, 100)]
    assert [(s.start, s.stop) for s in minibatch_slices(96, 48)] == [(0, 48), (48, 96)]
    assert [(s.start, s.stop) for s in minibatch_slices(5, 4096)] == [(0, 5)]
    with pytest.raises(ValueError):
        minibatch_slices(5, 0)


def test_near_float32_boundary_marks_midpoints_only():
    one, nxt = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))
    mid = (ref.LD(one) + ref.LD(nxt)) / 2
    x = np.array([mid, mid * (1 + ref.LD(2.0) ** -45), mid * (1 + ref.LD(2.0) ** -30), ref.LD(1.0), -mid], dtype=ref.LD)
    assert ref.near_float32_boundary(x).tolist() == [True, True, False, False, True]


def test_interface_is_declared_and_documented():
    import os
    from tum_control_amd import closed_loop, solver
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "tum_nmpc.h")).read()
    for word in ("tum_sim_ppo_attach", "tum_sim_ppo_step", "tum_sim_ppo_update", "tum_sim_ppo_params", "tum_sim_ppo_state", "TUM_PPO_STATS"):
        assert word in hdr and (word.startswith("TUM") or word in solver.C_SYMBOLS), word
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    for word in ("PPOTrainer", "closed_loop.learn", "float32 master", "perm"):
        assert word in doc, word
    for name in ("ppo_attach", "ppo_step", "ppo_update", "ppo_params", "ppo_state"):
        assert callable(getattr(solver.DeviceClosedLoop, name))
    for name in ("PPOTrainer", "learn", "ppo_loss_and_grads", "adam_step", "learning_rate_schedule"):
        assert hasattr(closed_loop, name)


def test_ppo_kernels_in_resource_table():
    """the five kernels are in the shipped library, the compiler reports no spills and no scratch for them, and policy_layers' KEEP
    variant left the two kernels that act at their register counts"""
    import os
    import shutil
    import __graft_entry__ as g
    if not (os.path.exists(g.HIPCC) or shutil.which("hipcc")) and not os.path.exists(g.LIB + ".resources"):
        pytest.skip("no hipcc and no resource table of a previous build on this host")
    g.build()
    rows = [line.split() for line in open(g.LIB + ".resources")]
    for name, max_vgpr in (("ppo_stats_kernel", 32), ("ppo_tile_kernel", 128), ("ppo_wgrad_kernel", 64), ("ppo_norm_kernel", 32),
                           ("ppo_adam_kernel", 48), ("policy_kernel", 76), ("policy_ac_kernel", 78)):
        hit = [r for r in rows if name in r[0]]
        assert len(hit) == 1, name
        vgpr, agpr, sgpr_spill, vgpr_spill, scratch, lds, occ = (int(x) for x in hit[0][1:])
        assert (sgpr_spill, vgpr_spill, scratch) == (0, 0, 0) and vgpr + agpr <= max_vgpr and lds <= 4096, (name, hit[0])
