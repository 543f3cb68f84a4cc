"""CPU guards around bench.py -- the one artefact the round is judged on (a NameError in a side leg
swallowed the JSON line).  Everything here runs without a GPU: the byte accounting, the cpu_baseline leg under every
flag that changes its inputs, the whole main() flow on the stub engine (TSVPP_BENCH_STUB=1: no kernels, a step is a
sleep), the --gpus N self-spawn on gloo, and the "not measured" line when fewer GPUs are visible than requested."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

REQUIRED = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "roofline"]


def _line(out):
    lines = [l for l in out.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, out
    return json.loads(lines[0])


def test_algorithmic_bytes_match_survey_8d():
    # SURVEY.md 8(d) "Per-config numbers"
    want = {"headline": 14169600, "c1": 4147200, "c2": 27993600, "c3": 2168832, "c4": 15206400, "c5": 15206400}
    for name, s in bench.WORKLOADS.items():
        assert bench.algorithmic_bytes(s[0], s[1], s[3], s[4], s[8]) == want[name], name
    assert bench.METRIC == json.load(open(os.path.join(ROOT, "BASELINE.json")))["metric"]


def test_touched_bytes_sparse_samplers():
    W = bench.WORKLOADS
    # dense samplers touch the whole ROI
    for name in ("headline", "c2", "c5"):
        s = W[name]
        assert bench.touched_bytes(s) == bench.algorithmic_bytes(s[0], s[1], s[3], s[4], s[8]), name
    # C3: wX == 0 (xF = 5 j + 2): one column per output column, two rows per output row
    assert bench.touched_bytes(W["c3"]) == 256 * 512 + 2 * 128 * 256 + 256 * 256 * 3 * 4
    # C4: bicubic at ratio 3 is a point sample: 1/9 of the source
    assert bench.touched_bytes(W["c4"]) == 3840 * 2160 * 3 // 2 // 9 + 1280 * 720 * 3
    s = list(W["headline"])
    s[5] = "NEAREST"
    assert bench.touched_bytes(tuple(s)) < bench.touched_bytes(W["headline"])


@pytest.mark.parametrize("tight", [False, True])
@pytest.mark.parametrize("rt,norm,planes", [("BILINEAR", True, "PLANAR"), ("AREA", False, "MERGED")])
def test_cpu_baseline_leg(tight, rt, norm, planes):
    spec = (320, 240, 512, (0, 0, 0, 0), (160, 120), rt, "BGR24", planes, norm)
    r = bench.cpu_baseline(spec, budget_s=0.2, tight_pitch=tight)
    assert r["value"] > 0 and r["unit"] == "frames/s" and r["cores"] >= 1 and r["kind"] == "port"
    assert r["swscale"] == "unavailable in image"


FLAG_SETS = [[], ["--tight-pitch"], ["--workload", "c4"], ["--workload", "c3", "--tight-pitch"], ["--resize", "AREA"],
             ["--custom", "640x360:320x180:BICUBIC:RGB24:MERGED:0"], ["--custom", "640x360:160x120:BILINEAR:RGB24:PLANAR:1:100,40,420,280"],   # (with a crop box)
             ["--per-call", "1"], ["--workload", "c5", "--no-others"]]


@pytest.mark.parametrize("flags", FLAG_SETS, ids=lambda f: " ".join(f) or "default")
def test_main_flow_on_the_stub_engine(flags, capsys, monkeypatch):
    """The --full path of main() (everything but the GPU engine): one well-formed line with roofline + cpu_baseline."""
    monkeypatch.setenv("TSVPP_BENCH_STUB", "1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    budget = "0.05" if ("c4" in flags or "c5" in flags) else "0.2"
    assert bench.main(["--full", "--steps", "3", "--warmup", "1", "--cpu-budget", budget] + flags) == 0
    res = _line(capsys.readouterr().out)
    for k in REQUIRED:
        assert k in res, k
    assert res["data"] == "stub" and res["n_gpus"] == 1 and res["steps"] == 3
    rf = res["roofline"]
    assert rf["bound"] == "hbm" and rf["peak"] == 8000.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    assert isinstance(rf["touched_bytes"], int) and "traffic_source" in rf
    reps = res["timing"]["repeats_ms_per_step"]
    assert len(reps) == 134 and res["timing"]["repeats"] == 134     # ceil(400 / 3 steps): at least 200 timed iterations, the clock ramp in the tail
    assert sorted(reps)[len(reps) // 2] == res["ms_per_step"]       # the median repeat
    cb = res["cpu_baseline"]
    assert "error" not in cb and cb["value"] > 0 and cb["swscale"] == "unavailable in image"
    if not flags:
        assert res["metric"] == bench.METRIC


def test_streams_flag_marks_the_line_as_a_diagnostic(capsys, monkeypatch):
    """--streams N overlaps launches: its figures are wall time per launch, so the line must say that it is not the contract's measurement."""
    monkeypatch.setenv("TSVPP_BENCH_STUB", "1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    assert bench.main(["--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-others", "--streams", "2"]) == 0
    res = _line(capsys.readouterr().out)
    assert res["data"].startswith("DIAGNOSTIC") and "2 streams" in res["data"]


def test_a_failing_side_leg_cannot_swallow_the_line(capsys, monkeypatch):
    monkeypatch.setenv("TSVPP_BENCH_STUB", "1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)

    def boom(*a, **k):
        raise NameError("name 'args' is not defined")

    monkeypatch.setattr(bench, "cpu_baseline", boom)
    monkeypatch.setattr(bench, "touched_bytes", boom)
    monkeypatch.setattr(bench, "lookup_traffic", boom)
    assert bench.main(["--full", "--steps", "2", "--warmup", "0"]) == 0
    res = _line(capsys.readouterr().out)
    assert "NameError" in res["cpu_baseline"]["error"] and res["value"] > 0
    assert "NameError" in res["roofline"]["touched_bytes"]["error"]


def test_gpus_2_self_spawn_on_gloo():
    """`python bench.py --gpus 2` without a torch.distributed environment re-executes itself under
    torch.distributed.run: rendezvous, barriers, max-over-ranks, ONE rank-0 line with n_gpus == 2."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["TSVPP_BENCH_STUB"] = "1"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1", "--full"],
                       env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    res = _line(p.stdout)
    assert res["n_gpus"] == 2 and res["value"] > 0 and res["scaling"] == "weak"
    assert res["per_rank"]["min_frames_per_s"] <= res["per_rank"]["max_frames_per_s"]
    assert abs(res["value"] - 2 * 64 * 4 / (res["ms_per_step"] * 4e-3)) / res["value"] < 1e-3  # whole-job aggregate
    # (round 6) N > 1 lines carry the CPU baseline too (rank 0, after the timed regions) and every rank's own roofline fraction
    assert res["cpu_baseline"]["value"] > 0 and res["cpu_baseline"]["kind"] == "port"
    assert len(res["per_rank"]["roofline_frac"]) == 2 and all(x > 0 for x in res["per_rank"]["roofline_frac"])


def test_gpus_more_than_visible_prints_not_measured():
    import torch
    n = (torch.cuda.device_count() if torch.cuda.is_available() else 0) + 1
    if n == 1:
        n = 2  # `--gpus 1` never spawns
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "TSVPP_BENCH_STUB")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n)], env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    res = _line(p.stdout)
    assert res["value"] is None and res["n_gpus"] == n and res["n_gpus_visible"] < n
    assert res["status"].startswith("not measured")


def test_stale_traffic_entries_are_dropped(tmp_path):
    p = tmp_path / "t.json"
    good = {"round": "rXX", "kernel_src_sha": bench.kernel_src_hash(), "frames_per_launch": 64.0, "hbm_bytes_per_launch": 123}
    p.write_text(json.dumps({"headline": good, "c2": dict(good, kernel_src_sha="0" * 16), "c5": {k: v for k, v in good.items() if k != "kernel_src_sha"}}))
    assert bench.lookup_traffic("headline", 64.0, str(p))[0] == 123
    assert bench.lookup_traffic("headline", 32.0, str(p))[0] is None
    for w in ("c2", "c5", "c3"):
        tr, why = bench.lookup_traffic(w, 64.0, str(p))
        assert tr is None and why
    # per-kernel stamps: valid while THAT kernel's translation unit and the shared headers are unchanged, and only for that kernel
    k = "tsvpp::vpp_bilinear_kernel<bilinear,OUT>"
    assert bench.kernel_source_files(k)[0].endswith("vpp_bilinear.hip") and bench.kernel_source_files("tsvpp::vpp_color_kernel<OUT>")[0].endswith("vpp_kernels.hip")
    assert bench.kernel_source_files("tsvpp::vpp_bilinear_r32_kernel<OUT,1,4>")[0].endswith("vpp_bilinear_r32.hip")
    p.write_text(json.dumps({"headline": dict(good, kernel=k, kernel_src_sha=bench.kernel_src_hash(k))}))
    assert bench.lookup_traffic("headline", 64.0, str(p), kernel=k)[0] == 123
    tr, why = bench.lookup_traffic("headline", 64.0, str(p), kernel="tsvpp::vpp_bicubic_int_kernel<OUT>")
    assert tr is None and "dispatches" in why


def _pmc_csv(path, counter, rows):
    """A rocprofv3 *_counter_collection.csv reduced to the columns the tools read."""
    with open(path, "w") as f:
        f.write('"Dispatch_Id","Kernel_Name","Counter_Name","Counter_Value"\n')
        for i, (k, v) in enumerate(rows):
            f.write(f'{i},"{k}","{counter}",{v}\n')


def test_traffic_entry_is_one_kernels_mean_not_a_blend(tmp_path):
    """round 3's tools averaged every tsvpp:: row; the headline entry was a blend of six kernels.  A CSV with two
    tsvpp kernels (+ a torch kernel) must reduce to the NAMED kernel's dispatches only."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pmc_lib
    import traffic_json
    hk = "void tsvpp::vpp_bilinear_kernel<false, 2>(tsvpp::LaunchDesc, tsvpp::FrameTable)"
    ok = "void tsvpp::vpp_area_box_kernel<6, true, 2>(tsvpp::LaunchDesc, tsvpp::FrameTable)"
    tk = "void at::native::vectorized_elementwise_kernel<4>(int)"
    _pmc_csv(tmp_path / "f.csv", "FETCH_SIZE", [(hk, 97300.0)] * 5 + [(ok, 389000.0)] * 9 + [(tk, 5.0)] * 3 + [(hk, 97302.0)] * 5)
    _pmc_csv(tmp_path / "w.csv", "WRITE_SIZE", [(hk, 691200.0)] * 10 + [(ok, 172800.0)] * 9 + [(tk, 7.0)] * 3)
    line = {"roofline": {"kernel": "tsvpp::vpp_bilinear_kernel<bilinear,OUT>", "bytes_per_frame": 14169600, "write_bytes_per_frame": 11059200},
            "config": {"frames_per_launch": 64.0}}
    e = traffic_json.entry("rXX", "headline", str(tmp_path / "f.csv"), str(tmp_path / "w.csv"), line, lambda k: "0" * 16)
    assert e["dispatches"] == 10 and e["kernel_csv_name"] == "tsvpp::vpp_bilinear_kernel<false, 2>"
    assert e["read_bytes"] == int(2 * 97301.0 * 1024) and e["write_bytes"] == 691200 * 1024
    assert e["algorithmic_write_bytes_per_launch"] == 11059200 * 64 and e["algorithmic_read_bytes_per_launch"] == 3110400 * 64
    # without a name: the tsvpp kernel with the most dispatches; a name that was never dispatched: nothing (never a blend)
    assert pmc_lib.pick_kernel(pmc_lib.load(str(tmp_path / "f.csv"))) == hk
    assert pmc_lib.pick_kernel(pmc_lib.load(str(tmp_path / "f.csv")), "tsvpp::vpp_color_kernel<OUT>") is None
    means, name = pmc_lib.kernel_means(pmc_lib.load(str(tmp_path / "w.csv")), "tsvpp::vpp_area_box_kernel<6,1,OUT>")
    assert name == ok and means["WRITE_SIZE"] == (172800.0, 9)
    with pytest.raises(SystemExit):
        traffic_json.entry("rXX", "c2", str(tmp_path / "f.csv"), str(tmp_path / "w.csv"), dict(line, roofline=dict(line["roofline"], kernel="tsvpp::vpp_color_kernel<OUT>")), lambda k: "0")


def test_implausible_traffic_entries_are_refused(tmp_path):
    """bench.py refuses an entry whose read or write side is more than 10 % off the algorithmic split unless touched_bytes explains it."""
    p = tmp_path / "t.json"
    base = {"round": "rXX", "kernel_src_sha": bench.kernel_src_hash(), "frames_per_launch": 64.0}
    alg_r, alg_w = 3110400 * 64, 11059200 * 64
    blend = dict(base, hbm_bytes_per_launch=911294239, read_bytes=341298378, write_bytes=569995860)  # round 3's published headline entry
    true = dict(base, hbm_bytes_per_launch=907100000, read_bytes=199270400, write_bytes=707812352, dispatches=659)
    p.write_text(json.dumps({"headline": blend}))
    tr, why = bench.lookup_traffic("headline", 64.0, str(p), alg_read=alg_r, alg_write=alg_w)
    assert tr is None and "implausible" in why
    p.write_text(json.dumps({"headline": true}))
    tr, why = bench.lookup_traffic("headline", 64.0, str(p), alg_read=alg_r, alg_write=alg_w)
    assert tr == 907100000 and "659 dispatches" in why
    # a sparse sampler (C4): reads far below the ROI bytes are accepted only down to the touched bytes
    c4 = bench.WORKLOADS["c4"]
    wr = 1280 * 720 * 3 * 64
    ar = (bench.algorithmic_bytes(c4[0], c4[1], c4[3], c4[4], c4[8]) - 1280 * 720 * 3) * 64
    tch = (bench.touched_bytes(c4) - 1280 * 720 * 3) * 64
    p.write_text(json.dumps({"c4": dict(base, hbm_bytes_per_launch=442481814, read_bytes=442481814 - wr, write_bytes=wr)}))
    tr, why = bench.lookup_traffic("c4", 64.0, str(p), alg_read=ar, alg_write=wr, touched_read=tch)
    assert tr == 442481814 and "touched_bytes" in why
    assert bench.lookup_traffic("c4", 64.0, str(p), alg_read=ar, alg_write=wr)[0] is None           # no explanation given
    p.write_text(json.dumps({"c4": dict(base, hbm_bytes_per_launch=1, read_bytes=tch // 2, write_bytes=wr)}))
    assert bench.lookup_traffic("c4", 64.0, str(p), alg_read=ar, alg_write=wr, touched_read=tch)[0] is None  # below what it must touch


def test_gpus_8_self_spawn_on_gloo():
    """The driver's SCALE run is the first time this code meets 8 ranks: rehearse the whole flow at world size 8 on gloo (stub engine):
    ONE line, n_gpus 8, eight per-rank entries, the 4K workloads in the line, whole-job aggregate."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["TSVPP_BENCH_STUB"] = "1"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "4", "--warmup", "1", "--full"],
                       env=env, capture_output=True, text=True, timeout=400)
    assert p.returncode == 0, p.stderr[-2000:]
    res = _line(p.stdout)
    assert res["n_gpus"] == 8 and res["value"] > 0 and res["scaling"] == "weak"
    pr = res["per_rank"]
    assert len(pr["frames_per_s"]) == 8 and len(pr["host_issue_ms_per_step"]) == 8 and all(x > 0 for x in pr["frames_per_s"])
    assert abs(res["value"] - 8 * 64 * 4 / (res["ms_per_step"] * 4e-3)) / res["value"] < 1e-3
    ow = res["config"]["other_workloads"]
    assert set(ow) == {"c1", "c2", "c3", "c4", "c5"} and all(ow[k]["frames_per_s"] > 0 for k in ow)
    assert res["cpu_baseline"]["value"] > 0 and len(pr["roofline_frac"]) == 8


def test_c5_as_baseline_words_it_64_named_consumers_over_8_ranks_on_gloo():
    """`--workload c5 --consumers 64 --gpus 8` -- 64 NAMED consumers, eight per rank, each rank its own converter; rehearsed at world 8 on gloo with
    the stub engine: one line, the consumer sharding in it, the aggregate = 64 conversions per step."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["TSVPP_BENCH_STUB"] = "1"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "4", "--warmup", "1", "--workload", "c5", "--consumers", "64",
                        "--cpu-budget", "0.05"], env=env, capture_output=True, text=True, timeout=400)
    assert p.returncode == 0, p.stderr[-2000:]
    res = _line(p.stdout)
    c = res["config"]["consumers"]
    assert res["n_gpus"] == 8 and c["total"] == 64 and c["per_rank"] == 8 and c["names_rank0"] == ["consumer0", "consumer7"]
    assert res["config"]["frames_per_step"] == 8 and abs(res["value"] - 8 * 8 * 4 / (res["ms_per_step"] * 4e-3)) / res["value"] < 1e-3
    assert len(res["per_rank"]["frames_per_s"]) == 8 and "other_workloads" not in res["config"]
    # a consumer count the ranks cannot share evenly is a set-up error, reported as ONE error line
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "2", "--warmup", "0", "--workload", "c5", "--consumers", "60"],
                       env=dict(env, TSVPP_BENCH_SETUP_TIMEOUT="20"), capture_output=True, text=True, timeout=240)
    assert p.returncode != 0 and '{"metric"' not in p.stdout and "not a multiple of the world size" in p.stdout


def test_torchrun_world1_takes_the_collective_path_on_gloo():
    """`torch.distributed.run --nproc-per-node=1 bench.py`: world size 1 still initialises the process group (the GPU twin of
    this test, tests/test_bench_gpu.py, runs the same on the nccl backend) -- one line, per_rank present."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["TSVPP_BENCH_STUB"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1", "--master-port", str(bench._free_port()),
           os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", "--no-cpu-baseline"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    res = _line(p.stdout)
    assert res["n_gpus"] == 1 and res["per_rank"]["backend"] == "gloo" and len(res["per_rank"]["host_issue_ms_per_step"]) == 1
    assert res["timing"]["total_timed_steps"] == res["timing"]["repeats"] * 4


@pytest.mark.parametrize("how,step", [("raise", "engine"), ("hang", "engine"), ("exit", "engine"), ("raise", "rendezvous")])
def test_a_rank_that_fails_its_setup_ends_the_job_with_one_error_line(how, step):
    """world size 8 on gloo, rank 5 fails in a set-up step (an exception, a hang, an abrupt exit): the job must end within a minute
    with ONE {"error": ...} line from rank 0 and a non-zero exit code -- never with seven ranks parked in a barrier."""
    import time
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env.update(TSVPP_BENCH_STUB="1", TSVPP_BENCH_FAIL=f"5:{step}:{how}", TSVPP_BENCH_SETUP_TIMEOUT="15")
    t0 = time.time()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "4", "--warmup", "1"], env=env, capture_output=True, text=True, timeout=240)
    took = time.time() - t0
    assert p.returncode != 0 and took < 90, (p.returncode, took, p.stderr[-1500:])
    assert '{"metric"' not in p.stdout
    lines = [l for l in p.stdout.splitlines() if l.startswith('{"error"')]
    assert len(lines) == 1, (p.stdout[-500:], p.stderr[-1500:])
    err = json.loads(lines[0])
    assert err["value"] is None and err["n_gpus"] == 8 and "set-up failed" in err["error"]
    assert "[bench.py rank 5/8]" in p.stderr  # every step of every rank is logged with its rank


def test_setup_times_travel_in_the_line():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["TSVPP_BENCH_STUB"] = "1"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1"], env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    res = _line(p.stdout)
    assert len(res["per_rank"]["setup_s"]) == 2 and all(x >= 0 for x in res["per_rank"]["setup_s"]) and res["timing"]["setup_s"] >= 0
    steps = [s[0] for s in res["per_rank"]["rank0_setup_steps"]]
    assert steps[:2] == ["rendezvous", "engine"] and "ready-check" in steps
    assert "set-up: rendezvous done" in p.stderr and "[bench.py rank 1/2]" in p.stderr


def test_plain_run_times_exactly_the_given_steps_and_nothing_else(capsys, monkeypatch):
    """Without --full: ONE timed region of exactly --steps steps, no side legs, no cpu_baseline, the parity gate left to --full."""
    monkeypatch.setenv("TSVPP_BENCH_STUB", "1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)

    def boom(*a, **k):
        raise AssertionError("a plain run must not run the cpu_baseline leg")

    monkeypatch.setattr(bench, "cpu_baseline", boom)
    assert bench.main(["--steps", "7", "--warmup", "2"]) == 0
    res = _line(capsys.readouterr().out)
    for k in REQUIRED:
        assert k in res, k
    t = res["timing"]
    assert res["steps"] == 7 and t["repeats"] == 1 and t["total_timed_steps"] == 7 and t["repeats_ms_per_step"] == [res["ms_per_step"]]
    assert abs(res["value"] - 64 * 7 / (res["ms_per_step"] * 7e-3)) / res["value"] < 1e-3
    assert "cpu_baseline" not in res and "other_workloads" not in res["config"] and "other_resize_types" not in res["config"]
    assert res["metric"] == bench.METRIC and res["higher_is_better"] is True and res["unit"] == "frames/s" and res["dtype"] == "f32"


def test_output_arrays_are_float32_within_64_mib():
    import torch
    small = torch.arange(2 * 3 * 8 * 8, dtype=torch.uint8).reshape(2, 3, 8, 8)
    a = bench.output_arrays(small)
    assert list(a) == ["output"] and a["output"].dtype == np.float32 and np.array_equal(a["output"], small.numpy().astype(np.float32))
    big = torch.rand((64, 3, 256, 1290), generator=torch.Generator().manual_seed(0))   # the headline's shape class: 254 MiB as float32
    a = bench.output_arrays(big)
    assert set(a) == {"output_frames", "output_frame_index", "output_sample"}
    assert sum(x.nbytes for x in a.values()) <= bench.DUMP_BYTES and all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert a["output_frame_index"].tolist() == [0, 31, 63] and np.array_equal(a["output_frames"], big[[0, 31, 63]].numpy())
    b = bench.output_arrays(big)   # the sample's positions are fixed: the same output gives the same arrays
    assert all(np.array_equal(a[k], b[k]) for k in a)
    huge = torch.zeros((4, 3, 2160, 3840), dtype=torch.uint8)     # a frame larger than the room beside the sample: the sample alone
    a = bench.output_arrays(huge)
    assert set(a) == {"output_sample"} and sum(x.nbytes for x in a.values()) <= bench.DUMP_BYTES


def test_dump_outputs_writes_the_last_step_the_same_way_every_run(tmp_path, capsys, monkeypatch):
    monkeypatch.setenv("TSVPP_BENCH_STUB", "1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    for run in ("a", "b"):
        assert bench.main(["--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / run)]) == 0
        res = _line(capsys.readouterr().out)
        assert res["config"]["dump_outputs"] == ["output"]
    a, b = np.load(tmp_path / "a" / "output.npy"), np.load(tmp_path / "b" / "output.npy")
    assert a.dtype == np.float32 and a.shape[0] == 64 and np.array_equal(a, b)
    with pytest.raises(SystemExit):   # a step of --consumers reads whatever frame the producer published last: nothing to compare
        bench.parse_args(["--workload", "c5", "--consumers", "8", "--dump-outputs", str(tmp_path / "c")])
