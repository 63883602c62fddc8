"""GPU: bench.py end to end on a small workload -- the JSON contract of the driver (fields, roofline and cpu_baseline
objects) and the quality of the result against the synthetic ground truth."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_contract_small():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1", "--full",
                        "--frames", "6", "--width", "1000", "--height", "750"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 1 and d["higher_is_better"] is True and d["vs_baseline"] is None and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"]
    rf = d["roofline"]
    # the line's roofline is the kernel that dominates the step that was run: at this toy size (6 frames of 0.75 MP) that may be either one,
    # at C3 it is the blur (6 levels of 12 MP per frame against one ransac launch of 499 pairs); both are always listed
    blur = rf if rf["kernel"].startswith("blur16_stream") else d["roofline_by_kernel"]["blur16_stream"]
    rk = d["roofline_by_kernel"]["ransac_kernel"]
    assert blur["bound"] == "valu" and blur["unit"] == "GB/s" and blur["peak"] == 8000.0 and abs(blur["frac"] - blur["achieved"] / blur["peak"]) < 1e-12
    assert blur["valu"]["frac"] > 0
    assert rk["bound"] == "valu" and rk["unit"] == "TFLOP/s" and rk["peak"] == 78.65 and abs(rk["frac"] - rk["achieved"] / rk["peak"]) < 1e-12
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12
    hf = d["host_frames"]
    assert hf["value"] > 0 and hf["pairs_accepted"] == 5 and "pageable host memory" in hf["sample"]      # what the adaptor's caller gets (host IplImages)
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0
    q = d["quality"]
    assert q["pairs"] == 5 and q["pairs_accepted"] == 5 and q["images_aligned"] == 6
    assert q["h_corner_err_px_median"] < 0.5
    assert d["value"] > 0


def _bench_line(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_bench_plain_run_is_the_headline_and_dumps_what_the_full_run_computes(tmp_path):
    """a plain run prints the headline line only (no rooflines, baselines or checks: those are --full's); --dump-outputs writes the
    last timed step's outputs, and a --full run with the same arguments computes the same ones"""
    import numpy as np
    small = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--frames", "6", "--width", "1000", "--height", "750"]
    d = _bench_line(small + ["--dump-outputs", str(tmp_path / "plain")])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 2 and d["value"] > 0 and abs(d["value"] - 5 / (d["ms_per_step"] / 1e3)) / d["value"] < 1e-6
    for k in ("roofline", "roofline_by_kernel", "cpu_baseline", "host_frames", "quality", "phase_ms", "parity_sample"):
        assert k not in d, k
    f = _bench_line(small + ["--full", "--no-cpu-baseline", "--no-host-frames", "--dump-outputs", str(tmp_path / "full")])
    assert f["quality"]["pairs_accepted"] == 5
    names = sorted(os.listdir(tmp_path / "plain"))
    assert names == sorted(os.listdir(tmp_path / "full")) and "canvas_sample.npy" in names and "pairs_H.npy" in names
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "plain" / n), np.load(tmp_path / "full" / n)
        assert a.dtype in (np.float32, np.float64) and a.dtype == b.dtype and a.shape == b.shape, n
        assert np.array_equal(a, b), n
        total += a.nbytes
    assert total <= 64 << 20
    p = np.load(tmp_path / "plain" / "pairs.npy")
    assert p.shape == (5, 6) and (p[:, 3] == 1).all()
    assert np.load(tmp_path / "plain" / "canvas_row_sums.npy").sum() > 0


def _two_ranks(extra, launcher=True):
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable]
    if launcher:
        cmd += ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port)]
    cmd += [os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1",
            "--width", "1000", "--height", "750", "--backend", "gloo", "--all-ranks-on-device0", "--full"] + extra
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line (rank 0)"
    assert r.stdout.strip().splitlines()[-1] == lines[0], "the JSON line is the last line of stdout"
    return json.loads(lines[0])


def test_bench_two_ranks_strong_dry_run_on_one_gpu():
    """the default N>1 path of bench.py: ONE survey, frames k mod 2 / pairs i mod 2 per rank, feature + result exchanges, canvas
    stripes, max-over-ranks timing, rank-0 JSON -- two processes sharing GPU 0, gloo standing in for RCCL (RCCL refuses two ranks on
    one device; the transport moves the same records through the same pack / install entry points)"""
    d = _two_ranks(["--frames", "9"])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["cpu_baseline"] is None
    assert d["config"]["frames"] == 9 and d["config"]["pairs"] == 8 and d["config"]["frames_per_gpu"] == 5 and d["config"]["pairs_per_gpu"] == 4
    assert d["quality"]["pairs_accepted"] == 8 and d["quality"]["images_aligned"] == 9 and d["quality"]["h_corner_err_px_median"] < 0.5
    # SURVEY 8e primary form: a rank holds the 5 (4) frames it extracts and receives the ones its canvas stripe reads; the alignment is
    # replicated from the moments and the records go to rank 0's host only
    assert d["frames_resident"].startswith("owned") and d["align_input"].startswith("moments")
    fx = d["frame_exchange_rank0"]
    assert fx["frames_held"] == 5 and fx["bytes_received"] > 0 and fx["bytes_sent"] > 0 and fx["frames_read_by_the_stripe"] <= 9      # (a single strip row: both horizontal stripes cross most frames)
    # whole-job aggregate: the survey's 8 pairs per step
    assert abs(d["value"] - 8 / (d["ms_per_step"] / 1e3)) / d["value"] < 1e-6


def test_bench_two_ranks_weak_dry_run_on_one_gpu():
    """--scaling weak: an independent strip per rank, the result all-gather only"""
    d = _two_ranks(["--frames", "5", "--scaling", "weak"])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["cpu_baseline"] is None
    assert d["config"]["pairs_per_gpu"] == 4 and d["quality"]["pairs_accepted"] == 4
    # whole-job aggregate: 2 ranks x 4 pairs per step
    assert abs(d["value"] - 8 / (d["ms_per_step"] / 1e3)) / d["value"] < 1e-6


def test_bench_plain_command_form_launches_its_ranks():
    """`python bench.py --gpus 2` with no launcher environment (the driver's command form) must run TWO ranks, not silently one
    (VERDICT r02): bench.py re-executes itself under torch.distributed.run.  The line names the transport; rccl_ranks is null
    because gloo / torch transport carries this one-device dry run."""
    d = _two_ranks(["--frames", "9"], launcher=False)
    assert d["n_gpus"] == 2 and d["scaling"] == "strong"
    assert d["transport"] == "torch" and d["rccl_ranks"] is None
    assert d["config"]["frames_per_gpu"] == 5 and d["quality"]["pairs_accepted"] == 8


def test_bench_two_ranks_replicas_and_records_forms_still_run():
    """the round-5 forms stay selectable: every frame on every rank (no exchange) and the records all-gathered to every rank"""
    d = _two_ranks(["--frames", "9", "--frames-resident", "replicas", "--align-input", "records"])
    assert d["frames_resident"] == "all frames on every rank" and d["align_input"] == "records" and "frame_exchange_rank0" not in d
    assert d["quality"]["pairs_accepted"] == 8 and d["quality"]["images_aligned"] == 9


def test_bench_window_line_quotes_the_kernel_that_dominates():
    """with the reference's pair window the pair stage outweighs detect+describe: the line's roofline is ransac_kernel's, against the
    f32 vector peak, from the counted lane-operation formula"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-host-frames",
                        "--frames", "150", "--width", "640", "--height", "480", "--window", "182"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    rf = d["roofline"]
    assert rf["kernel"].startswith("ransac_kernel") and rf["bound"] == "valu" and rf["unit"] == "TFLOP/s" and rf["peak"] == 78.65
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12 and 0 < rf["frac"] < 1
    assert rf["us_per_pair"] > 0 and rf["lane_ops_per_pair_mean"] > 1e6
    assert d["roofline_by_kernel"]["blur16_stream"]["bound"] == "valu" and d["mfma"]["kernel"] == "bf_match_kernel"
