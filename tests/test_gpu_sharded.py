"""-m gpu: time-sharded windows (BASELINE.json configs[4] at test size): one window
spread over 2 ranks, each owning half of the chunks of the partitioned solve.  The box has one GPU,
so both ranks share it and the collectives run over gloo (host-staged); on a multi-GPU node the
same ShardedSolver uses RCCL.  Gate: same trajectory as the unsharded engine (the arithmetic is
identical up to the order of the cost sum) and ATE <= 1e-6 m against the oracle."""
import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

from tests import helpers
from vil_sensor_fusion_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N, CHUNKS, ITERS = 400, 8, 5


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _problem():
    from oracle import oracle
    oracle.build()
    seq = synth.make_sequence(seed=21, n_kf=N)
    return oracle, helpers.build_problem(oracle, seq, perturb=0.01)


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch
    from vil_sensor_fusion_amd import Engine, EngineOpts, distributed as D
    dist = D.init(backend="gloo")
    _, prob = _problem()
    eng = Engine(EngineOpts(windows=1, capacity=N + 8, chunks=CHUNKS))
    helpers.load_engine(eng, 0, prob)
    solver = D.ShardedSolver(eng, dist, "cuda:0", backend="gloo")
    solver.iterate(ITERS)
    torch.cuda.synchronize()
    assert solver.collectives == 2 * ITERS          # one all-gather + one all-reduce per LM trial, none for the cost
    q.put((rank, eng.get_states(0, 0, N), eng.read_lm(0)))
    D.barrier(dist)
    dist.destroy_process_group()


def test_two_ranks_share_one_window():
    from vil_sensor_fusion_amd import Engine, EngineOpts
    oracle, prob = _problem()
    ref = Engine(EngineOpts(windows=1, capacity=N + 8, chunks=CHUNKS))
    helpers.load_engine(ref, 0, prob)
    ref.iterate(ITERS)
    ref_states, ref_lm = ref.get_states(0, 0, N), ref.read_lm(0)
    ref.close()

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=300) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    (r0, s0, lm0), (r1, s1, lm1) = res
    np.testing.assert_array_equal(s0, s1)                      # replicated state stays identical on the ranks
    assert lm0 == lm1
    d, _ = helpers.ate(s0, ref_states)
    worst = float(np.abs(s0 - ref_states).max())
    print(f"2 ranks vs 1: ATE {d:.3e} m, largest state difference {worst:.3e}; lm {lm0} vs {ref_lm}")
    assert d <= 1e-9 and worst <= 1e-9     # (2 acos|q.q'| cannot resolve below 4e-8 rad: compare the components)
    assert lm0["accepted"] == ref_lm["accepted"] and lm0["solve_failures"] == 0
    win = helpers.oracle_window(oracle, prob)
    win.lm(iterations=ITERS)
    a, r = helpers.ate(s0, win.states)
    print(f"2 ranks vs oracle: ATE {a:.3e} m")
    assert a <= 1e-6 and r <= 1e-6


def test_single_rank_sharded_solver_equals_engine_iterate():
    """world = 1: ShardedSolver drives the same stages as vf_engine_iterate (no collectives)."""
    import torch
    from vil_sensor_fusion_amd import Engine, EngineOpts, distributed as D
    _, prob = _problem()
    out = []
    for sharded in (False, True):
        eng = Engine(EngineOpts(windows=1, capacity=N + 8, chunks=CHUNKS))
        helpers.load_engine(eng, 0, prob)
        if sharded:
            D.ShardedSolver(eng, None, "cuda:0").iterate(ITERS)
            torch.cuda.synchronize()
        else:
            eng.iterate(ITERS)
        out.append((eng.get_states(0, 0, N), eng.read_lm(0)))
        eng.close()
    np.testing.assert_array_equal(out[0][0], out[1][0])
    assert out[0][1] == out[1][1]


def _rccl_worker(port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      VF_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch
    from vil_sensor_fusion_amd import Engine, EngineOpts, distributed as D
    torch.cuda.set_device(0)
    dist = D.init(backend="nccl", device_id=torch.device("cuda", 0))
    assert dist is not None and dist.get_backend() == "nccl"
    _, prob = _problem()
    eng = Engine(EngineOpts(windows=1, capacity=N + 8, chunks=CHUNKS))
    helpers.load_engine(eng, 0, prob)
    solver = D.ShardedSolver(eng, dist, "cuda:0", backend="nccl")
    solver.iterate(ITERS)
    torch.cuda.synchronize()
    q.put((eng.get_states(0, 0, N), eng.read_lm(0), solver.collectives))
    D.barrier(dist)
    dist.destroy_process_group()


def test_rccl_code_path_one_rank():
    """The nccl (= RCCL) branch of the exchange -- in-place all_gather_into_tensor of the packed separator buffer and the
    all_reduce of [increments | failure flags] on the engine's stream -- on hardware, with a world of one rank
    (VF_FORCE_DIST=1): same states as vf_engine_iterate, bit for bit, and exactly two collectives per LM trial."""
    from vil_sensor_fusion_amd import Engine, EngineOpts
    _, prob = _problem()
    ref = Engine(EngineOpts(windows=1, capacity=N + 8, chunks=CHUNKS))
    helpers.load_engine(ref, 0, prob)
    ref.iterate(ITERS)
    ref_states, ref_lm = ref.get_states(0, 0, N), ref.read_lm(0)
    ref.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_worker, args=(_free_port(), q))
    p.start()
    states, lm, ncoll = q.get(timeout=300)
    p.join(timeout=120)
    assert p.exitcode == 0
    np.testing.assert_array_equal(states, ref_states)
    assert lm == ref_lm
    assert ncoll == 2 * ITERS


def test_bench_gpus_flag_starts_that_many_ranks(tmp_path):
    """`python bench.py --gpus 2` (no WORLD_SIZE): bench.py itself starts two ranks; here they share the box's one GPU and
    talk over gloo.  The line must say n_gpus 2 and carry roofline, the detail file the time-sharded section's two collectives
    per trial."""
    import json
    import subprocess
    env = dict(os.environ, VF_BENCH_BACKEND="gloo", VF_BENCH_SHARE_GPU="1", VF_BENCH_DETAIL_DIR=str(tmp_path))
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--windows", "8", "--window", "96", "--steps", "2",
           "--warmup", "1", "--sharded-window", "1200", "--no-single-window"]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-2000:]
    text = [l for l in res.stdout.splitlines() if l.startswith("{")][-1]
    line = json.loads(text)
    assert len(text) < 4096 and line["n_gpus"] == 2 and line["value"] > 0
    assert line["roofline"]["bound"] == "hbm" and 0 < line["roofline"]["frac"] < 1 and "cpu_baseline" not in line    # (the CPU legs are timed at N = 1 only)
    assert line["time_sharded_window"]["ranks"] == 2 and line["detail"] == "bench_detail.json"
    sh = json.load(open(tmp_path / "bench_detail.json"))["time_sharded_window"]
    assert "error" not in sh, sh
    assert sh["ranks"] == 2 and sh["collectives_per_trial"] == 2
    assert sh["collectives_issued"] == 2 * sh["lm_trials_run"] and sh["solve_failures"] == 0


def test_bench_abandons_a_stalled_sharded_section():
    """A multi-rank run whose time-sharded section gives no result in time (here: a limit of zero seconds) must still hand
    the driver the headline: every rank leaves, rank 0 prints the line it has, and the exit status says that the
    collective section hung (bench.EXIT_SHARDED_SECTION_HUNG) -- a stalled exchange is not a success."""
    import json
    import subprocess
    env = dict(os.environ, VF_BENCH_BACKEND="gloo", VF_BENCH_SHARE_GPU="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--windows", "8", "--window", "96", "--steps", "2",
           "--warmup", "1", "--sharded-window", "1200", "--no-single-window", "--sharded-timeout", "0"]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 75, (res.returncode, res.stderr[-2000:])
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["value"] > 0 and line["ms_per_step"] > 0
    assert "error" in line["time_sharded_window"]
    assert line["roofline"]["bound"] == "hbm" and 0 < line["roofline"]["frac"] < 1      # (the fallback line carries the roofline too)


# ---------------------------------------------------------------- BASELINE configs[4] at its real geometry
N4, CHUNKS4, ITERS4, REFINE4 = 10000, 96, 10, 12     # (a window this long runs refined solves by default: 12 corrections each)


def _problem4():
    from oracle import oracle
    oracle.build()
    seq = synth.make_sequence(seed=5, n_kf=N4)
    return oracle, helpers.build_problem(oracle, seq)


def test_config4_eight_shards_of_twelve_chunks_vs_oracle():
    """The 10 000-pose window cut into 96 chunks, owned 12 each by EIGHT shards -- the geometry of the 8-GPU run.  The pool
    gives one GPU and at most six GPU processes, so the eight shards are eight engines of one process
    (distributed.LockstepGroup: ShardedSolver's own phases, the two collectives of a trial carried out between the engines'
    device buffers).  The window is past what float64 normal equations resolve, so every solve is refined through J (the
    library's default for it; 12 corrections = 12 more solves, two collectives each) and the accept rule is the
    non-monotone one; ten trials converge it from dead reckoning.  Gates: all shards hold identical states, equal to the
    unsharded engine to 1e-7 m (ATE), ATE <= 1e-6 m against the oracle doing the same, 2 x (1 + 12) collectives per trial."""
    import torch
    from vil_sensor_fusion_amd import Engine, EngineOpts, distributed as D
    oracle, prob = _problem4()
    ref = Engine(EngineOpts(windows=1, capacity=N4 + 8, chunks=CHUNKS4))
    helpers.load_engine(ref, 0, prob)
    ref.iterate(ITERS4)
    ref_states, ref_lm = ref.get_states(0, 0, N4), ref.read_lm(0)
    ref.close()
    world = 8
    engines = []
    for r in range(world):
        e = Engine(EngineOpts(windows=1, capacity=N4 + 8, chunks=CHUNKS4))
        helpers.load_engine(e, 0, prob)
        engines.append(e)
    owned = [D.shard_range(N4, CHUNKS4, r, world) for r in range(world)]
    assert [o[1] - o[0] for o in owned] == [12] * 8 and owned[0][2] == 0 and owned[-1][3] == N4
    assert all(owned[r][3] == owned[r + 1][2] for r in range(world - 1))          # the keyframe ranges tile the window
    group = D.LockstepGroup(engines, "cuda:0")
    group.iterate(ITERS4)
    torch.cuda.synchronize()
    assert engines[0].refine_count() == REFINE4 and group.collectives == 2 * (1 + REFINE4) * ITERS4
    states = [e.get_states(0, 0, N4) for e in engines]
    lms = [e.read_lm(0) for e in engines]
    for r in range(1, world):
        np.testing.assert_array_equal(states[r], states[0])
        assert lms[r] == lms[0]
    # (two converged refined solves of a window whose softest modes sit at the rounding floor: compared as trajectories)
    worst = helpers.ate(states[0], ref_states)[0]
    assert worst <= 1e-7 and lms[0]["accepted"] == ref_lm["accepted"] and lms[0]["solve_failures"] == 0
    win = helpers.oracle_window(oracle, prob)
    costs, acc, _ = win.lm(iterations=ITERS4, refine=REFINE4, excursion=3)
    a, rot = helpers.ate(states[0], win.states)
    print(f"8 shards x 12 chunks, {N4} poses: vs unsharded ATE {worst:.3e} m; vs oracle ATE {a:.3e} m rot {rot:.3e} rad; "
          f"cost {lms[0]['cost']:.9e} oracle {costs[-1]:.9e}")
    assert a <= 1e-6 and rot <= 1e-6
    assert abs(lms[0]["cost"] - costs[-1]) <= 1e-9 * abs(costs[-1])
    for e in engines:
        e.close()


GLOO_REFINE, GLOO_UPDATES = 3, 2


def _worker4(rank, world, port, q, prob):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch
    from vil_sensor_fusion_amd import Engine, EngineOpts, distributed as D
    dist = D.init(backend="gloo")
    eng = Engine(EngineOpts(windows=1, capacity=N4 + 8, chunks=CHUNKS4, refine_iterations=GLOO_REFINE))
    helpers.load_engine(eng, 0, prob)
    solver = D.ShardedSolver(eng, dist, "cuda:0", backend="gloo")
    for _ in range(GLOO_UPDATES):
        solver.gn_step(0.0)
    torch.cuda.synchronize()
    assert solver.collectives == 2 * (1 + GLOO_REFINE) * GLOO_UPDATES
    st = eng.get_estimate(0, 0, N4)
    q.put((rank, st if rank == 0 else float(np.abs(st).sum())))
    D.barrier(dist)
    dist.destroy_process_group()


def test_config4_four_processes_over_gloo():
    """The same 10 000-pose window, 96 chunks, as FOUR real ranks (24 chunks each) in four processes sharing the box's GPU,
    exchanging over gloo -- as many processes as the pool's limit of six on the card leaves room for beside the test
    runner.  The process boundary, the rendezvous and the collectives are real; only the transport is not RCCL.  Two
    reference-compat updates (Gauss-Newton), each solve refined by three corrections = 16 collectives; four processes
    taking turns on one GPU are slow, so convergence is the lock-step test's business (above) and this one checks the
    arithmetic: the ranks end with identical estimates, bit for bit those of four lock-step shards in ONE process."""
    import torch
    from vil_sensor_fusion_amd import Engine, EngineOpts, distributed as D
    oracle, prob = _problem4()
    world = 4
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker4, args=(r, world, port, q, prob)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=600) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    s0 = res[0][1]
    for r in range(1, world):
        assert res[r][1] == float(np.abs(s0).sum())                                  # identical replicated estimates
    engines = []
    for r in range(world):
        e = Engine(EngineOpts(windows=1, capacity=N4 + 8, chunks=CHUNKS4, refine_iterations=GLOO_REFINE))
        helpers.load_engine(e, 0, prob)
        engines.append(e)
    group = D.LockstepGroup(engines, "cuda:0")
    for _ in range(GLOO_UPDATES):
        group.gn_step(0.0)
    torch.cuda.synchronize()
    lock = engines[0].get_estimate(0, 0, N4)
    worst = float(np.abs(lock - s0).max())
    print(f"4 ranks x 24 chunks over gloo, {N4} poses, {GLOO_UPDATES} refined Gauss-Newton updates: largest difference from four lock-step shards {worst:.3e}")
    np.testing.assert_array_equal(lock, s0)
    for e in engines:
        e.close()


def test_shard_errors():
    from vil_sensor_fusion_amd import Engine, EngineOpts
    from vil_sensor_fusion_amd._lib import VilFusionError
    eng = Engine(EngineOpts(windows=1, capacity=64, chunks=1))
    with pytest.raises(VilFusionError):
        eng.set_shard(0, 2)                      # sweeps cannot be sharded
    with pytest.raises(VilFusionError):
        eng.shard_info()                         # no separator buffers without the partitioned solve
    with pytest.raises(VilFusionError):
        eng.solve_local()
    with pytest.raises(VilFusionError):
        eng.set_convergence(-1.0, 0.0)
    eng.set_shard(0, 1)                          # a world of one is always fine
    eng.close()
    eng = Engine(EngineOpts(windows=1, capacity=64))            # chunks chosen by the engine: not shardable either
    with pytest.raises(VilFusionError):
        eng.set_shard(0, 2)
    eng.close()
    eng = Engine(EngineOpts(windows=1, capacity=64, chunks=6))
    with pytest.raises(VilFusionError):
        eng.set_shard(0, 4)                      # 6 chunks over 4 ranks
    with pytest.raises(VilFusionError):
        eng.set_shard(2, 2)
    eng.set_shard(1, 2)
    eng.set_range(0, 0, 20)
    with pytest.raises(VilFusionError):
        eng.solve_local()                        # 20 keyframes cannot hold 6 chunks
    for whole_window_call in (lambda: eng.iterate(1), eng.solve, eng.marginalize):
        with pytest.raises(VilFusionError):
            whole_window_call()                  # a shard cannot run whole-window stages on its own
    eng.close()


def test_config4_shards_take_the_same_decisions_through_failed_excursions():
    """The non-monotone rule on a time-sharded window: every rank evaluates the whole cost and must take the same decision --
    provisional, accepted, restored (the saved states come back and the factors of EVERY rank are linearised again) -- as the
    unsharded engine.  lm_excursion = 1 makes the 10 000-pose window alternate provisional trial / restore (tests/
    test_gpu_vs_qr_twin.py::test_config4_a_failed_excursion_restores_the_point_it_left); four shards in lock step."""
    import torch
    from vil_sensor_fusion_amd import Engine, EngineOpts, distributed as D
    oracle, prob = _problem4()
    K = 9
    ref = Engine(EngineOpts(windows=1, capacity=N4 + 8, chunks=CHUNKS4, lm_excursion=1))
    helpers.load_engine(ref, 0, prob)
    ref.iterate(K)
    want = (ref.read_lm(0), ref.read_excursions(0), ref.get_states(0, 0, N4))
    ref.close()
    engines = []
    for r in range(4):
        e = Engine(EngineOpts(windows=1, capacity=N4 + 8, chunks=CHUNKS4, lm_excursion=1))
        helpers.load_engine(e, 0, prob)
        engines.append(e)
    group = D.LockstepGroup(engines, "cuda:0")
    group.iterate(K)
    torch.cuda.synchronize()
    got = [(e.read_lm(0), e.read_excursions(0), e.get_states(0, 0, N4)) for e in engines]
    for r in range(1, 4):
        assert got[r][0] == got[0][0] and got[r][1] == got[0][1]
        np.testing.assert_array_equal(got[r][2], got[0][2])
    a = helpers.ate(got[0][2], want[2])[0]
    print(f"4 shards, lm_excursion = 1, {K} trials: {got[0][0]}, provisional {got[0][1]}; unsharded: {want[0]}, {want[1]}; ATE {a:.3e} m")
    assert want[0]["rejected"] >= 2 and want[1][0] >= 3                        # the restore path ran
    assert {k: got[0][0][k] for k in ("accepted", "rejected", "solve_failures")} == {k: want[0][k] for k in ("accepted", "rejected", "solve_failures")}
    assert got[0][1] == want[1] and a <= 1e-3
    for e in engines:
        e.close()
