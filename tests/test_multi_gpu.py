"""Multi-GPU plumbing: round-robin frame sharding and the one-time calibration-table
broadcast.  The data path has no collective; the broadcast is the
caller's torch.distributed backend -- RCCL ("nccl") on GPUs, gloo here: world_size 2 on CPU.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_round_robin_sharding_covers_every_frame_once():
    from mono_dataset_code_amd import shard

    for n, world in ((50000, 8), (17, 4), (3, 8), (0, 2), (1024, 1)):
        seen = np.zeros(n, np.int32)
        for r in range(world):
            fr = shard.frames_of_rank(n, r, world)
            assert len(fr) == shard.count_of_rank(n, r, world)
            assert all(shard.owner_of(int(f), world) == r for f in fr)
            assert [shard.local_index(int(f), world) for f in fr] == list(range(len(fr)))
            seen[fr] += 1
        assert np.all(seen == 1)
    # config 4 of BASELINE.json: 50k frames over 8 GPUs -> 6250 each
    assert [shard.count_of_rank(50000, r, 8) for r in range(8)] == [6250] * 8


WORKER = r'''
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np, torch, torch.distributed as dist
from mono_dataset_code_amd import capi, shard
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%(port)d", rank=rank, world_size=world)
d = %(calib)r
blob = None
if rank == 0:   # only rank 0 touches the calibration files
    fov = capi.UndistorterFOV(os.path.join(d, "camera.txt"))
    photo = capi.PhotometricUndistorter(os.path.join(d, "pcalib.txt"), os.path.join(d, "vignette.png"), *fov.dims()[:2])
    blob = capi.pack_tables(fov, photo)
got = shard.broadcast_tables(blob, src=0)
# every rank ends with the same bytes; rank 1 cross-checks against tables it builds itself
digest = torch.tensor([int(np.frombuffer(got.tobytes(), np.uint8).astype(np.uint64).sum()), got.size], dtype=torch.int64)
all_d = [torch.zeros_like(digest) for _ in range(world)]
dist.all_gather(all_d, digest)
assert all(torch.equal(all_d[0], x) for x in all_d), all_d
if rank == 1:
    fov = capi.UndistorterFOV(os.path.join(d, "camera.txt"))
    photo = capi.PhotometricUndistorter(os.path.join(d, "pcalib.txt"), os.path.join(d, "vignette.png"), *fov.dims()[:2])
    assert np.array_equal(capi.pack_tables(fov, photo), got)
# the shard arithmetic bench.py uses
mine = shard.frames_of_rank(37, rank, world)
cnt = torch.tensor([len(mine)]); dist.all_reduce(cnt); assert int(cnt) == 37
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok", got.size)
'''


def test_table_broadcast_gloo_world2(calib_dirs, tmp_path):
    script = tmp_path / "worker.py"
    port = 29500 + (os.getpid() % 500)
    script.write_text(WORKER % {"root": ROOT, "port": port, "calib": calib_dirs["small_crop"]})
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=240)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, o[-3000:])
        assert "rank %d ok" % r in o


@pytest.mark.gpu
def test_packed_blob_equals_exported_blob(calib_dirs):
    """Host-side pack (what rank 0 broadcasts) == device context export, and importing it
    reproduces the context."""
    from mono_dataset_code_amd import capi

    d = calib_dirs["small_explicit"]
    fov = capi.UndistorterFOV(os.path.join(d, "camera.txt"))
    photo = capi.PhotometricUndistorter(os.path.join(d, "pcalib.txt"), os.path.join(d, "vignette.png"), *fov.dims()[:2])
    ctx = capi.Context(0)
    ctx.bind(fov, photo)
    packed = capi.pack_tables(fov, photo)
    assert np.array_equal(packed, ctx.export_tables())
    c2 = capi.Context(0)
    c2.import_tables(packed)
    assert np.array_equal(c2.export_tables(), packed)
    i1, i2 = ctx.info(), c2.info()
    assert (i1.in_w, i1.out_w, i1.tiled, i1.n_tiles, i1.src_bbox_bytes) == (i2.in_w, i2.out_w, i2.tiled, i2.n_tiles, i2.src_bbox_bytes)


def _bench(args, env=None, nproc=0, port=29533, timeout=900, clean_env=False):
    import json

    e = dict(os.environ, MASTER_ADDR="127.0.0.1") if not clean_env else {}
    e.update(env or {})
    if nproc:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.join(ROOT, "bench.py")] + args
    else:
        cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + args
    r = subprocess.run(cmd, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]  # gloo announces itself on stdout, ranks interleaved
    assert len(lines) == 1, r.stdout  # exactly one JSON line, from rank 0
    return json.loads(lines[0])


def _check_rank_dumps(dump_dir, world, n, oracle):
    """Every rank's first n outputs against the oracle for the GLOBAL frame index rank + i * world, recomputed here
    from the frame generator: the frame -> rank mapping is checked on bytes, not on arithmetic."""
    from conftest import bits_equal
    from mono_dataset_code_amd import capi, synth

    d = synth.write_sequence_calibration(tempfile.mkdtemp(prefix="mdc_dump_"))
    fov = capi.UndistorterFOV(os.path.join(d, "camera.txt"))
    photo = capi.PhotometricUndistorter(os.path.join(d, "pcalib.txt"), os.path.join(d, "vignette.png"), 1280, 1024)
    rx, ry = fov.remap()
    ginv, vinv = photo.ginv(), photo.vignette()[1]
    for r in range(world):
        out = np.load(os.path.join(dump_dir, "rank%d_out.npy" % r))
        idx = np.load(os.path.join(dump_dir, "rank%d_idx.npy" % r))
        head = np.load(os.path.join(dump_dir, "rank%d_in_head.npy" % r)).reshape(n, 64)
        assert out.shape == (n, 640 * 480) and list(idx) == [r + i * world for i in range(n)]
        for i in range(n):
            raw = synth.noise_frames(int(idx[i]), 1, 1280 * 1024)[0]
            assert np.array_equal(head[i], raw[:64]), "rank %d local frame %d does not hold global frame %d" % (r, i, idx[i])
            want = oracle.get_image(raw, 1280, 1024, 640, 480, ginv, vinv, True, True, rx, ry, 1, 1, 1, 1)
            assert bits_equal(out[i], want), (r, i, int(idx[i]))


@pytest.mark.gpu
def test_bench_two_ranks_on_one_gpu(tmp_path, oracle):
    """bench.py's N>1 path end to end (rank-0 table build, broadcast, import on every rank, round-robin
    shard, barrier + max-over-ranks timing, one JSON line from rank 0) with two ranks sharing the one GPU
    of the test box: gloo carries the collectives there (RCCL wants one device per rank).  EVERY rank's first
    three outputs are compared with the oracle for their global frame indices."""
    out = _bench(["--full", "--gpus", "2", "--steps", "5", "--warmup", "2", "--frames", "64", "--preroll-s", "0.05", "--preroll-max-s", "0.2",
                  "--dump-dir", str(tmp_path), "--dump-frames", "3"], env={"MDC_BENCH_BACKEND": "gloo"}, nproc=2)
    assert out["n_gpus"] == 2 and out["scaling"] == "weak" and out["steps"] == 5
    assert out["config"]["frames_per_gpu_per_step"] == 64 and "cpu_baseline" not in out
    assert out["parity"]["mismatching_pixels"] == 0
    assert out["config"]["tables"].startswith("rank-0 build") and out["config"]["collective_backend"] == "gloo"
    assert len(out["roofline"]["per_rank_kernel_ms_mean_median_min"]) == 2
    _check_rank_dumps(str(tmp_path), 2, 3, oracle)


@pytest.mark.gpu
def test_bench_launches_its_own_ranks(tmp_path, oracle):
    """`python bench.py --gpus 2` WITHOUT torchrun becomes two ranks by itself (gloo here: the two ranks share the test box's one
    GPU) and says so in its line; without the gloo switch it refuses to run more ranks than there are GPUs -- it never prints
    n_gpus: 1 for --gpus N."""
    import torch

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    out = _bench(["--full", "--gpus", "2", "--steps", "4", "--warmup", "1", "--frames", "64", "--preroll-s", "0.05", "--preroll-max-s", "0.2", "--dump-dir", str(tmp_path),
                  "--dump-frames", "2"], env=dict(env, MDC_BENCH_BACKEND="gloo"), clean_env=True)
    assert out["n_gpus"] == 2 and out["ranks"]["world"] == 2 and out["ranks"]["backend"] == "gloo"
    assert [d["rank"] for d in out["ranks"]["devices"]] == [0, 1]
    assert out["parity"]["mismatching_pixels"] == 0 and len(out["roofline"]["per_rank_frac"]) == 2
    assert out["build_flags"] == ""
    _check_rank_dumps(str(tmp_path), 2, 2, oracle)
    want = torch.cuda.device_count() + 1
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(want), "--frames", "8", "--steps", "1", "--warmup", "0"],
                       env=dict(env, MDC_BENCH_BACKEND="nccl"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0 and "GPU(s) visible" in r.stderr and not [l for l in r.stdout.splitlines() if l.startswith("{")]
    # a launcher that disagrees with --gpus is an error as well, whatever the world size
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--frames", "8", "--steps", "1", "--warmup", "0"],
                       env=dict(env, WORLD_SIZE="1", RANK="0"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr


@pytest.mark.gpu
def test_bench_seq50k_sharding_two_ranks(tmp_path, oracle):
    """BASELINE.json configs[3] (one sequence, frame f on GPU f % N), shrunk to 2 x 40 frames: strong scaling line,
    per-rank outputs equal to the oracle for the global indices."""
    out = _bench(["--full", "--gpus", "2", "--steps", "3", "--warmup", "1", "--workload", "seq50k", "--frames", "40", "--preroll-s", "0.05", "--preroll-max-s", "0.2",
                  "--dump-dir", str(tmp_path), "--dump-frames", "2", "--no-ceiling"], env={"MDC_BENCH_BACKEND": "gloo"}, nproc=2, port=29537)
    assert out["scaling"] == "strong" and out["config"]["sequence_frames"] == 80 and out["config"]["frames_per_gpu_per_step"] == 40
    assert out["parity"]["mismatching_pixels"] == 0
    _check_rank_dumps(str(tmp_path), 2, 2, oracle)


@pytest.mark.gpu
def test_bench_rccl_branch_executes_with_a_world_of_one(tmp_path):
    """The "nccl" (= RCCL) branch of bench.py on the one GPU of the test box: process-group init on the device, the
    table broadcast, the barriers and the all-reduce / all-gather all run through RCCL with world size 1."""
    out = _bench(["--full", "--gpus", "1", "--steps", "4", "--warmup", "1", "--frames", "128", "--preroll-s", "0.05", "--preroll-max-s", "0.2", "--no-cpu-baseline"],
                 env={"MDC_BENCH_FORCE_DIST": "1", "MDC_BENCH_BACKEND": "nccl", "RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0",
                      "MASTER_PORT": "29539"})
    assert out["n_gpus"] == 1 and out["config"]["collective_backend"] == "nccl"
    assert out["config"]["tables"] == "rank-0 build + one RCCL broadcast"
    assert out["parity"]["mismatching_pixels"] == 0
    assert out["roofline"]["frac_of_same_box_mix_ceiling"] > 0.3 and out["roofline"]["kernel"].startswith("remap_tiled_kernel<")
    # the table broadcast itself ran through RCCL (a world of one does not skip it under MDC_BENCH_FORCE_DIST): 7.7 MB, timed
    assert out["config"]["table_blob_bytes"] > 7_000_000 and out["config"]["table_broadcast_ms"] > 0
    assert len(out["roofline"]["per_rank_frac"]) == 1 and out["roofline"]["per_rank_frac"][0] > 0.1


@pytest.mark.gpu
def test_bench_pyramid_checks_every_level():
    out = _bench(["--full", "--steps", "3", "--warmup", "1", "--workload", "pyramid", "--frames", "16", "--preroll-s", "0.05", "--preroll-max-s", "0.2", "--no-cpu-baseline"])
    par = out["parity"]
    assert (par["frames_checked"], par["levels_checked"], par["mismatching_pixels"]) == (16, 4, 0)  # --frames 16: every frame of the launch
    # base against the reference build where it was built (else the C oracle, pinned to the reference's recorded answers); the levels' definition is ours
    from oracle import loader

    assert ("libmdc_ref.so" if loader.have_ref() else "liboracle.so") in par["against"] and "unpinned" in par["pinned"]
    assert out["roofline"]["kernel"].startswith("remap_strip_kernel<true, true")  # the strip kernel with the fused pyramid ran


@pytest.mark.gpu
def test_bench_over_rccl_on_real_devices(tmp_path, oracle):
    """The first run on a multi-GPU node must need no edits: with >= 2 visible devices, `python bench.py --gpus N` (the driver's
    form: it launches its own ranks) runs N = 2 and N = all over RCCL -- every rank on a device of its own (distinct PCI
    addresses), rccl_ranks == N, every rank's outputs == the oracle for their GLOBAL frame indices f = rank + i * N --, and the one
    50,000-frame-style sequence (configs[3], shrunk) is dealt round-robin with every rank reporting.  Skips on one device, where
    test_bench_two_ranks_on_one_gpu (gloo, shared GPU) and test_bench_rccl_world_of_one cover the same code."""
    import torch

    ndev = torch.cuda.device_count()
    if ndev < 2:
        pytest.skip("one visible device: RCCL across devices needs two")
    for n in sorted({2, ndev}):
        dump = tmp_path / ("dump%d" % n)
        dump.mkdir()
        out = _bench(["--full", "--gpus", str(n), "--steps", "5", "--warmup", "2", "--frames", "256", "--preroll-s", "0.05", "--preroll-max-s", "0.3",
                      "--dump-dir", str(dump), "--dump-frames", "3", "--no-cpu-baseline"], clean_env=False, timeout=1200)
        ranks = out["ranks"]
        assert out["n_gpus"] == n and ranks["world"] == n and ranks["backend"] == "nccl" and ranks["rccl_ranks"] == n
        assert [d["device"] for d in ranks["devices"]] == list(range(n))
        assert len({d["pci"] for d in ranks["devices"]}) == n, ranks["devices"]  # N ranks, N different GPUs
        assert out["parity"]["mismatching_pixels"] == 0 and len(out["roofline"]["per_rank_frac"]) == n
        assert out["config"]["tables"] == "rank-0 build + one RCCL broadcast" and out["config"]["table_broadcast_ms"] > 0
        # every rank allocates through the product's allocator on ITS device and says what it got
        for d_ in ranks["devices"]:
            assert d_["placement"]["strategy"] in ("first", "malloc", "vmm"), d_
        _check_rank_dumps(str(dump), n, 3, oracle)
        seq = _bench(["--full", "--gpus", str(n), "--steps", "3", "--warmup", "1", "--workload", "seq50k", "--frames", "96", "--preroll-s", "0.05", "--preroll-max-s",
                      "0.3", "--no-cpu-baseline"], timeout=1200)
        assert seq["scaling"] == "strong" and seq["config"]["sequence_frames"] == 96 * n and seq["parity"]["mismatching_pixels"] == 0
        assert seq["ranks"]["rccl_ranks"] == n and len(seq["roofline"]["per_rank_frac"]) == n


@pytest.mark.gpu
@pytest.mark.parametrize("strategy", ["malloc", "vmm"])
def test_bench_takes_its_buffers_from_the_product_allocator(strategy):
    """bench.py has no buffer search of its own: frames and results come from mdc_alloc_placed_device (libmdc_hip.so), whose report -- the
    strategy, what it timed, the probe on the first allocations beside the probe on the pair handed out -- goes into the line."""
    env = {"MDC_PLACE_SPREAD_MB": "2000", "MDC_PLACE_PIECE_MIB": "256"}
    out = _bench(["--full", "--steps", "4", "--warmup", "1", "--frames", "1024", "--placement", strategy, "--placement-candidates", "3", "--preroll-s", "0.05",
                  "--preroll-max-s", "0.3", "--no-cpu-baseline", "--no-secondary"], env=env)
    pl = out["config"]["placement"]
    assert pl["strategy"] == strategy and pl["probe_frames"] == 1024 and pl["ms_on_chosen_pair"] > 0
    if strategy == "malloc":
        m = pl["ms_frames_i_results_j"]
        assert len(m) == 3 and all(len(r) == 3 for r in m) and all(0 < x < 20 for r in m for x in r)
        assert m[pl["picked_frames"]][pl["picked_results"]] == min(x for r in m for x in r)
    else:
        assert sum(pl["class_count"]) == pl["pieces"] >= 11 and pl["piece_mib"] == 256
    assert out["parity"]["mismatching_pixels"] == 0 and out["parity"]["frames_checked"] == 16
    assert (out["parity"]["nan_mask_mismatches"], out["parity"]["black_pixel_mismatches"], out["parity"]["max_relative_error"]) == (0, 0, 0.0)
    rp = out["roofline"]["placement"]
    assert rp["probe_ms_on_chosen_pair"] == pl["ms_on_chosen_pair"]
    if rp["probe_ms_on_first_allocations"]:
        assert 0.2 < rp["frac_on_first_allocation"] < 0.9
    assert out["ranks"]["devices"][0]["placement"]["strategy"] == strategy
    assert 0.2 < out["roofline"]["frac"] < 0.9
    plain = _bench(["--full", "--steps", "4", "--warmup", "1", "--frames", "1024", "--placement", "first", "--preroll-s", "0.05", "--preroll-max-s", "0.3",
                    "--no-cpu-baseline", "--no-secondary"])
    assert plain["config"]["placement"]["strategy"] == "first" and plain["parity"]["mismatching_pixels"] == 0


@pytest.mark.gpu
def test_bench_plain_run_is_the_headline_alone():
    """Without --full the line carries the headline and nothing that takes runs or checks of its own -- no same-box ceiling, no parity,
    no other configs, no second timing, no CPU reference --, on the headline's own batch of 4096 frames, where --full adds them all."""
    out = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--preroll-s", "0.05", "--preroll-max-s", "0.3"])
    assert (out["metric"], out["unit"], out["higher_is_better"], out["dtype"]) == ("Mpix/s photometric+FOV undistort, 1280x1024 gray", "Mpix/s", True, "f32")
    assert out["steps"] == 3 and out["warmup"] == 1 and out["config"]["frames_per_gpu_per_step"] == 4096
    assert out["value"] == pytest.approx(4096 * 1280 * 1024 / 1e6 / (out["ms_per_step"] * 1e-3), rel=1e-3)
    assert not {"secondary", "again", "cpu_baseline"} & set(out), sorted(out)
    assert not {"same_box_mix_ceiling", "frac_of_same_box_mix_ceiling", "frac_again"} & set(out["roofline"])
    assert isinstance(out["parity"], str) and "--full" in out["parity"]
    assert out["roofline"]["kernel"].startswith("remap_tiled_kernel<") and 0.2 < out["roofline"]["frac"] < 0.9


def _dump_check(dump_dir, workload, world, oracle, stride=None):
    """bench.py --dump-outputs: every file float32 / float64 and finite, all together under 64 MB; per rank, the base image of every
    listed frame -- value where the non-finite code is 0, NaN / +inf / -inf where it says so -- equals the oracle's for that GLOBAL frame
    index (every `stride`-th element where a frame is sampled).  -> {file name: bytes}"""
    from conftest import bits_equal
    from mono_dataset_code_amd import capi, synth

    files = sorted(os.listdir(dump_dir))
    assert sum(os.path.getsize(os.path.join(dump_dir, f)) for f in files) <= 64 * 1000 * 1000
    got = {}
    for f in files:
        a = np.load(os.path.join(dump_dir, f))
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f
        got[f] = a
    pyr = workload in ("pyramid", "dso")
    lines = synth.camera_lines(1280, 1024, 1280, 1024) if pyr else synth.CAMERA_1280_TO_640
    d = synth.write_sequence_calibration(tempfile.mkdtemp(prefix="mdc_dump_"), lines)
    fov = capi.UndistorterFOV(os.path.join(d, "camera.txt"))
    photo = capi.PhotometricUndistorter(os.path.join(d, "pcalib.txt"), os.path.join(d, "vignette.png"), 1280, 1024)
    (rx, ry), ginv, vinv = fov.remap(), photo.ginv(), photo.vignette()[1]
    ow, oh = fov.dims()[2:]
    for r in range(world):
        p = "rank%d_" % r if world > 1 else ""
        frames = got[p + "frames.npy"]
        v, code = got[p + "out.npy"].copy(), got[p + "out_nonfinite.npy"]
        assert set(np.unique(code)) <= {0, 1, 2, 3} and np.all(v[code != 0] == 0)
        v[code == 1], v[code == 2], v[code == 3] = np.nan, np.inf, -np.inf
        assert len(frames) == v.shape[0] >= 1 and len(set(frames.tolist())) == len(frames)
        for i, f in enumerate(frames):
            assert f == int(f) and int(f) % world == r, (r, f)  # round-robin: rank r holds the global frames r, r + N, ...
            raw = synth.noise_frames(int(f), 1, 1280 * 1024)[0]
            want = oracle.get_image(raw, 1280, 1024, ow, oh, ginv, vinv, True, True, rx, ry, 1, 1, 1, 1)
            assert bits_equal(v[i], want[::stride] if stride else want), (workload, r, int(f))
    return {f: open(os.path.join(dump_dir, f), "rb").read() for f in files}


@pytest.mark.gpu
def test_bench_dump_outputs_repeat_and_match_the_oracle(tmp_path, oracle):
    """Two runs of the headline with the same arguments write the same files, byte for byte, and the sampled frames are the oracle's."""
    args = ["--full", "--steps", "3", "--warmup", "1", "--frames", "64", "--preroll-s", "0.05", "--preroll-max-s", "0.2", "--no-cpu-baseline", "--no-ceiling"]
    dumps = []
    for run in ("a", "b"):
        out = _bench(args + ["--dump-outputs", str(tmp_path / run)])
        assert out["steps"] == 3 and out["parity"]["mismatching_pixels"] == 0
        dumps.append(_dump_check(str(tmp_path / run), "fused", 1, oracle))
    assert sorted(dumps[0]) == ["frames.npy", "out.npy", "out_nonfinite.npy"]
    assert dumps[0] == dumps[1]
    assert np.load(str(tmp_path / "a" / "out_nonfinite.npy")).any()  # the overexposed pixels of the noise frames are there, coded


@pytest.mark.gpu
@pytest.mark.parametrize("workload,world,frames,stride", [("pyramid", 1, 8, None), ("dso", 1, 4, 2), ("dso", 2, 4, 3)])
def test_bench_dump_outputs_stay_within_64_mb(tmp_path, oracle, workload, world, frames, stride):
    """The larger workloads, one rank and two (gloo, sharing the GPU): every output array is written (levels, gradient images), the
    whole directory stays under 64 MB, a frame too large on its own is sampled every `stride`-th element, and the base images are the oracle's."""
    args = ["--steps", "2", "--warmup", "1", "--workload", workload, "--frames", str(frames), "--preroll-s", "0.05", "--preroll-max-s", "0.2",
            "--no-cpu-baseline", "--no-ceiling", "--dump-outputs", str(tmp_path)]
    if world == 1:
        _bench(args)
    else:
        _bench(["--gpus", str(world)] + args, env={"MDC_BENCH_BACKEND": "gloo"}, nproc=world, port=29543)
    dump = _dump_check(str(tmp_path), workload, world, oracle, stride)
    names = ["out", "level1", "level2", "level3"] + (["dI%d" % l for l in range(4)] + ["abs%d" % l for l in range(4)] if workload == "dso" else [])
    prefixes = ["rank%d_" % r for r in range(world)] if world > 1 else [""]
    assert sorted(dump) == sorted([p + "frames.npy" for p in prefixes] + [p + n + s for p in prefixes for n in names for s in (".npy", "_nonfinite.npy")])
