"""CPU: the bench line's contract -- its headline dtype is the one the product runs, and its roofline
traffic comes from the committed PMC summary of the same workload (bench.py pmc_traffic)."""
import sys


def test_headline_dtype_is_the_product_default(monkeypatch):
    import inspect

    import bench
    from mopo_amd.bnn import DEFAULT_ENSEMBLE_DTYPE
    from mopo_amd.mopo import MOPO
    monkeypatch.setattr(sys, 'argv', ['bench.py'])
    args = bench.parse()
    assert args.ensemble_dtype == DEFAULT_ENSEMBLE_DTYPE
    # MOPO builds its ensemble with DEFAULT_ENSEMBLE_DTYPE unless ensemble_dtype is passed
    assert inspect.signature(MOPO.__init__).parameters['ensemble_dtype'].default is None
    assert 'DEFAULT_ENSEMBLE_DTYPE' in inspect.getsource(MOPO.__init__)


def test_committed_pmc_summary_prices_the_measured_workloads(monkeypatch):
    import bench
    for argv, lo in ((['bench.py'], 19.6e6), (['bench.py', '--ensemble-dtype', 'fp32'], 19.6e6),
                     (['bench.py', '--config', 'N2'], 31.7e6)):
        monkeypatch.setattr(sys, 'argv', argv)
        args = bench.parse()
        t = bench.pmc_traffic(args)
        assert t is not None and t > 0, 'profiles PMC summary has no pass for %s' % bench.workload_key(args)
        # HBM bytes per ensemble launch: at least the algorithmic bytes, far below 1 GB
        alg = bench.ensemble_bytes(args.batch, bench.CONFIGS[args.config], args.ensemble_dtype)
        assert alg >= lo * 0.9 and alg * 0.9 <= t < 1e9, (bench.workload_key(args), alg, t)


def test_cpu_baseline_median_of_five_after_warmup():
    """every CPU-baseline figure is the median of >= 5 timed runs after 1 warm-up."""
    import bench
    calls = []

    def fn():
        calls.append(1)
        return 10, 0.5 + 0.1 * len(calls)
    med, runs, units, secs = bench.median_runs(fn)
    assert len(calls) == 1 + bench.CPU_RUNS and len(runs) == bench.CPU_RUNS >= 5
    assert med == sorted(runs)[len(runs) // 2] and units == 10 * bench.CPU_RUNS
    run = bench.cpu_rollout_leg(64, 2, 'walker2d', 5.0, env_rows=500)   # the oracle rollout leg, tiny
    n, dt = run()
    assert 0 < n <= 128 and dt > 0


def test_roofline_names_the_dispatched_ensemble_kernel():
    """The roofline's kernel is the one csrc/bnn.hip launch_bnn_fwd dispatches at the config's width: the LDS ring
    at H <= 256 (bf16x6: P = 3, f16x3: P = 2), the column-half f16h kernel for f16x3 at H = 400, the split bf16
    kernel for bf16x6 at H = 400; the executed-flop fraction counts every MFMA product."""
    import bench
    ms, rows = 0.5, 50000
    r = bench.roofline_of('bf16x6', rows, ms, bench.FLOP_BNN_ROW, 200)
    assert r['kernel'].startswith('bnn_fwd_ring_kernel<P=3>')
    assert abs(r['frac'] - 6 * rows * bench.FLOP_BNN_ROW / (ms * 1e-3) / 1e12 / bench.BF16_PEAK_TFLOPS) < 1e-12
    assert bench.roofline_of('f16x3', rows, ms, bench.FLOP_BNN_ROW, 200)['kernel'].startswith('bnn_fwd_ring_kernel<P=2>')
    assert bench.roofline_of('f16x3', rows, ms, bench.FLOP_BNN_ROW, 400)['kernel'].startswith('bnn_fwd_f16h_kernel')
    assert bench.roofline_of('bf16x6', rows, ms, bench.FLOP_BNN_ROW, 400)['kernel'].startswith('bnn_fwd_bf16_kernel<P=3>')
    assert bench.roofline_of('fp32', rows, ms)['kernel'].startswith('bnn_fwd_kernel')


def test_plain_run_is_the_default_and_full_is_an_option(monkeypatch):
    import bench
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '7', '--warmup', '2'])
    args = bench.parse()
    assert args.full is False and args.dump_outputs is None and args.steps == 7 and args.warmup == 2
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--full', '--dump-outputs', 'd'])
    args = bench.parse()
    assert args.full is True and args.dump_outputs == 'd'
    line = bench.headline(args, 1, 5000000, 0.05)
    assert line['value'] == 1e8 and line['unit'] == 'transitions/s' and line['higher_is_better'] is True
    assert abs(line['ms_per_step'] - 50.0 / args.steps) < 1e-12 and 'halfcheetah-mixed' in line['metric']
    assert line['dtype'] == bench.dtype_desc(args.ensemble_dtype)


def test_dump_outputs_writes_the_last_rollouts_rows(tmp_path, monkeypatch):
    """--dump-outputs: the last n rows of the pool's ring in append order, float32 (steps_added float64), and past
    the byte limit the same seeded sample of them on every run."""
    import numpy as np
    import torch

    import bench
    from mopo_amd.replay_pool import FIELDS, SimpleReplayPool
    pool = SimpleReplayPool(obs_dim=3, act_dim=2, max_size=10, device='cpu')
    for j, k in enumerate(FIELDS):
        v = pool.fields[k]
        rows = torch.arange(10).reshape(10, 1).expand(10, v.shape[1])
        pool.fields[k] = (rows % 2 == 0) if v.dtype == torch.bool else (rows + 100.0 * j).to(v.dtype)
    pool._state[0], pool._state[1] = 2, 10      # wrapped: the last 6 rows appended are 6, 7, 8, 9, 0, 1
    steps = torch.tensor([4, 2])
    bench.dump_outputs(str(tmp_path / 'a'), steps, pool)
    got = {k: np.load(str(tmp_path / 'a' / (k + '.npy'))) for k in FIELDS + ('steps_added',)}
    assert got['steps_added'].dtype == np.float64 and got['steps_added'].tolist() == [4.0, 2.0]
    assert all(got[k].dtype == np.float32 and got[k].shape == (6, pool.fields[k].shape[1]) for k in FIELDS)
    assert got['observations'][:, 0].tolist() == [6, 7, 8, 9, 0, 1]
    assert got['next_observations'][:, 2].tolist() == [406, 407, 408, 409, 400, 401]
    assert got['terminals'][:, 0].tolist() == [1, 0, 1, 0, 1, 0]
    monkeypatch.setattr(bench, 'DUMP_LIMIT', 8192 + 4 * 10 * 3)   # 10 values a row: room for 3 rows
    bench.dump_outputs(str(tmp_path / 'b'), steps, pool)
    bench.dump_outputs(str(tmp_path / 'c'), steps, pool)
    b, c = (np.load(str(tmp_path / d / 'observations.npy'))[:, 0].tolist() for d in 'bc')
    order = [6, 7, 8, 9, 0, 1]
    assert b == c and len(b) == 3 and [order.index(x) for x in b] == sorted(order.index(x) for x in b)
    assert np.load(str(tmp_path / 'b' / 'actions.npy'))[:, 0].tolist() == [x + 100 for x in b]
