#!/usr/bin/env python3
"""bench.py -- headline benchmark: CIRIM inference throughput (slices/sec) on synthetic fastMRI-knee-shaped data.

Workload (BASELINE.json `metric`): CIRIM, 8 cascades x 8 time-steps (config time_steps 5 is rounded up to 8 by the model,
reference cirim.py:50-51), IndRNN 64 filters, 15 coils, 640x372, fp32, batch 1 slice per GPU (the reference default).
A "step" is one full reconstruction of one batch through the HIP path (64 RIM steps = 384 kernel launches).

    python bench.py --gpus N --steps K --warmup W
One process per GPU (the reference: pytorch-lightning `strategy: ddp`, base_cirim_train.yaml:175).  Under torch.distributed.run the
ranks exist already (WORLD_SIZE / RANK / LOCAL_RANK in the environment); a bare `python bench.py --gpus N` with N > 1 spawns the N
rank processes itself -- from a parent that never touches the GPU -- and exits with their status.  Slices shard across ranks with
no data-path collective ("weak" scaling); timing is barrier + synchronize on both sides, max over ranks; rank 0 prints the line,
with the world size RCCL reported and every rank's own time so a straggler is visible.

A plain run sets up, warms up, times the K steps and prints ONE JSON line with the contract fields (metric, value, unit,
higher_is_better, dtype, ms_per_step, ...).  `--full` adds what takes runs of its own:
  roofline      dominant kernel (fused conv3x3(d2)+IndRNN layer, fp32 MFMA): algorithmic FLOPs / HIP-event time
  roofline_fft  the FFT+DC step (log_likelihood_gradient) against the HBM roofline, (25+16C)*H*W bytes per slice-step
  cpu_baseline  the CPU oracle (restatement of the reference's torch-CPU path) on a bounded sample, rank 0, N=1 only
  and the concurrent-replay check, the streamed-input figure and the other configurations (`other_configs`, `exact_fp32_route`).
`--dump-outputs DIR` writes what the timed path returned in its last step as DIR/<name>.npy (float32 / float64, <= 64 MB in all).
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_FP32_MFMA_TFLOPS = 157.3   # /opt/skills/guides/MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 peak
PEAK_BF16_MFMA_TFLOPS = 2500.0  # same guide: dense bf16 (v_mfma_f32_32x32x16_bf16), no sparsity
PEAK_HBM_GBS = 8000.0           # HBM3E spec peak


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=0, help="slices per stream per step (0 = the measured best per model: 1, E2EVN and CIRIM inference 8)")
    ap.add_argument("--streams", type=int, default=0,
                    help="independent slice batches reconstructed concurrently per GPU, one HIP stream + one captured hipGraph each "
                         "(slices are independent: two in flight fill each other's launch tails and stalls; 1 = single stream; "
                         "0 = the measured best per model: 2 (qCIRIM: 6); E2EVN (batch x streams) 1 x 3 / 2 x 2 / 3 x 2 / 4 x 2: 644 / 677 / 701 / 721 slices/s -- its "
                         "small-grid kernels overlap their load / matrix / store phases only when a launch spans several dispatch rounds; CIRIM's "
                         "persistent kernels gain nothing from batching: 88.2 / 88.8 / 88.9 / 86.7 at 1 x 2 / 2 x 2 / 4 x 2 / 8 x 1)")
    ap.add_argument("--coils", type=int, default=15)
    ap.add_argument("--height", type=int, default=640)
    ap.add_argument("--width", type=int, default=372)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--train-graph", type=int, default=0, help="CIRIM training: forward + backward of the explicit tape as one hipGraph replay (training.GraphedCirimStep; measured 45.3 ms against 43.1 ms eager on two streams: the step is not launch-bound, off by default)")
    ap.add_argument("--graph", type=int, default=1, help="replay the step as a captured hipGraph (falls back to eager)")
    ap.add_argument("--model", default="cirim", choices=["cirim", "e2evn", "qcirim", "rvn", "ccnn", "vsnet"],
                    help="cirim = the headline workload (BASELINE.json metric); e2evn = configs[1], reported for reference")
    ap.add_argument("--mask", default="1d", choices=["1d", "2d"],
                    help="1d: random columns R=4 (SURVEY 8d primary); 2d: random 2-D points R=10 (stands in for the YAML's Poisson-2D)")
    ap.add_argument("--rnn", default="IndRNN", choices=["IndRNN", "GRU", "MGU"],
                    help="recurrent layer of the CIRIM cascades (headline: IndRNN; GRU with --cascades 1 is the reference's RIM config)")
    ap.add_argument("--cascades", type=int, default=0, help="override num_cascades (0 = the headline's 8)")
    ap.add_argument("--rim-steps", type=int, default=0,
                    help="time-steps per RIMBlock call (0 = CIRIM's own: config time_steps 5 rounded up to 8, models/cirim.py:50-51); 5 = what a direct "
                         "RIMBlock(time_steps=5) runs (models/rim/rim_block.py:68,217) -- SURVEY 0.4 asks for both figures")
    ap.add_argument("--train", action="store_true",
                    help="config C4: data-parallel TRAINING steps of the CIRIM (forward, l1 loss, backward through the HIP kernels, one "
                         "flat-gradient all-reduce, Adam) instead of inference; fp32")
    ap.add_argument("--cpu-cascades", type=int, default=0,
                    help="cascades of the CPU-baseline sample (0 = all of them: one whole slice, about 20 s on the GPU box's host)")
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16"],
                    help="--train only: bf16 = convolution / IndRNN GEMM operands in bf16 with fp32 accumulation (the reference's "
                         "`precision: 16` AMP, base_cirim_train.yaml:180), FFT / data consistency / eta accumulation stay fp32")
    ap.add_argument("--precision", type=int, default=32, choices=[32, 16],
                    help="inference precision: 16 = the reference's own inference configuration (`trainer.precision: 16` in every *_run.yaml of its model zoo, e.g. "
                         "base_cirim_run.yaml:132 = torch.autocast(float16) around forward).  --model cirim: fp16 operands and fp16 hidden states in both RIM layers "
                         "(csrc/rim_amp16.hip); --model e2evn / qcirim: the 3x3 convolutions on one fp16 term (mrx_unet_conv3x3_p16 / mrx_conv3x3_p16); other models: "
                         "ignored (fp32-class).  Checked against the oracle under torch.autocast(float16).  Never the headline: the default run reports these as "
                         "other_configs.*_precision16_*")
    ap.add_argument("--unet", default="14x2", choices=["14x2", "18x4"],
                    help="--model e2evn: NormUnet(chans x pools): 14x2 pad 11 = BASELINE configs[1]; 18x4 pad 15 = the reference yaml's default")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="headline only: skip the short E2EVN-6 / qCIRIM / bf16-training runs and the exact-route child that the default N = 1 "
                         "run adds to its line as `other_configs` / `exact_fp32_route`")
    ap.add_argument("--stream-inputs", action="store_true", help=argparse.SUPPRESS)      # (the default since round 4; kept so old command lines parse)
    ap.add_argument("--no-stream-inputs", action="store_true",
                    help="skip the second headline figure `streamed_inputs`: a NEW (y, S, mask) per slice streamed from pinned host memory on a copy "
                         "stream while the previous slice reconstructs (models/base.py:638-713: the reference feeds every slice through a DataLoader)")
    ap.add_argument("--cpu-slices", type=int, default=3,
                    help="timed slices of the CPU-baseline leg after its warm-up (BASELINE.md section 3: >= 3; mean and min are reported)")
    ap.add_argument("--dist-selftest", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline figure: HIP-event kernel breakdown and rooflines, the concurrent-replay check, the CPU baseline "
                         "and parity against the oracle, the streamed-input figure and the other configurations (each still switched off by its --no-* flag)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path returned in its last step as DIR/<name>.npy (float32 / float64, at most "
                         "64 MB in all: larger outputs as a fixed, seeded sample); rank 0 only")
    args = ap.parse_args()
    args.stream_inputs = not args.no_stream_inputs
    if args.streams <= 0:
        args.streams = 6 if (args.model == "qcirim" and not args.train) else 2     # (qCIRIM on 4 / 6 / 8 streams: 740 / 790 / 781 slices/s, tools/runs/r06x.sh)
    if args.batch <= 0:
        # CIRIM inference: 480 tiles of 16 x 32 pixels per slice on 256 CUs -- 8 slices per launch are exactly 15 rounds of the persistent layer kernels
        # (one slice: two rounds, the second 7/8 full); measured 1 x 2 / 2 x 2 / 4 x 2 / 8 x 2 / 8 x 1 / 16 x 1 (batch x streams), lib 252:
        # 140.7 / 141.3 / 142.9 / 144.1 / 134.7 / 134.7 slices/s (2-D masks: 101.1 / 104.6 / 100.7 at 1 / 4 / 8 x 2: 4 -- at 8 the 228-MB coil stack of the three-pass gradient no longer fits the 256-MB Infinity Cache)
        # E2EVN (batch x streams, lib 252): 4 x 2 1023, 6 x 2 1087, 8 x 2 1103-1109, 10 x 2 1109, 12 x 2 1108, 16 x 2 1081, 8 x 3 1101, 8 x 1 925, 16 x 1 985
        args.batch = 8 if (args.model == "e2evn" and not args.train) else (8 if args.mask == "1d" else 4) if (args.model == "cirim" and not args.train and args.rnn == "IndRNN") else 1
    return args


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def rank_launch_plan(n_gpus, argv, environ):
    """The N child (command, environment) pairs of a bare `--gpus N` run, or None when this process is a rank already (a launcher
    set WORLD_SIZE) or N == 1.  Pure host logic: nothing here may touch the GPU (the children initialise it, never the parent)."""
    if n_gpus <= 1 or "WORLD_SIZE" in environ:
        return None
    port = environ.get("MASTER_PORT") or str(_free_port())
    plan = []
    for r in range(n_gpus):
        env = dict(environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n_gpus), LOCAL_WORLD_SIZE=str(n_gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL between processes needs it on this driver
        plan.append(([sys.executable, os.path.abspath(__file__)] + list(argv), env))
    return plan


def spawn_ranks(plan):
    """Start every rank as a fresh child, wait for all; if one fails stop the others (exact PIDs) and return its status."""
    import subprocess
    procs = [subprocess.Popen(cmd, env=env) for cmd, env in plan]
    rc = 0
    try:
        pending = list(procs)
        while pending:
            for p_ in list(pending):
                r = p_.poll()
                if r is None:
                    continue
                pending.remove(p_)
                if r != 0 and rc == 0:
                    rc = r
                    for q in pending:
                        q.terminate()
            time.sleep(0.05)
    finally:
        for p_ in procs:
            if p_.poll() is None:
                p_.kill()
    return rc


def dist_selftest(args):
    """`--dist-selftest`: the rank plumbing of this file (process-group init, barrier, max over ranks, per-rank times) on the gloo
    backend with no GPU work -- what tests/test_sharding_gloo.py runs to cover the spawn path on a CPU-only machine."""
    import torch.distributed as dist
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from mridc_amd.sharding import shard_range
    s0, s1 = shard_range(world * 2, rank, world)
    dist_barrier(sync=False)
    t0 = time.perf_counter()
    time.sleep(0.01 * (rank + 1))
    dist_barrier(sync=False)
    elapsed, per_rank = rank_times(time.perf_counter() - t0, None)
    if rank == 0:
        print(json.dumps(dict(selftest="dist", n_gpus=world, gpus_flag=args.gpus, world_size_seen=dist.get_world_size() if world > 1 else 1,
                              per_rank_ms=[1e3 * t for t in per_rank], max_ms=1e3 * elapsed, slices_rank0=[s0, s1])), flush=True)
    if world > 1:
        dist.destroy_process_group()


class KernelTimer:
    """HIP events around every launch of selected ops (recorded on the stream the kernels are launched on)."""

    def __init__(self):
        self.events = {}
        self.enabled = False

    def wrap(self, module, name, key_fn):
        orig = getattr(module, name)
        timer = self

        def wrapped(*a, **k):
            key = key_fn(*a, **k) if timer.enabled else None
            if key is None:
                return orig(*a, **k)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            r = orig(*a, **k)
            e.record()
            timer.events.setdefault(key, []).append((s, e))
            return r

        setattr(module, name, wrapped)

    def calibrate(self, n=64):
        """Half the elapsed time of an EMPTY event pair = the closing event's own processing time on the command processor (~2.4 us on this
        stack: an empty pair reads 4.8 us).  Every bracketed launch carries exactly that much on top of the kernel; mean_ms subtracts it, so
        the event figures agree with rocprofv3's kernel durations (the raw mean is kept as raw_ms)."""
        pairs = []
        for _ in range(n):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            e.record()
            pairs.append((s, e))
        torch.cuda.synchronize()
        t = sorted(s.elapsed_time(e) for s, e in pairs)
        self.pair_ms = t[len(t) // 2]
        return self.pair_ms

    def raw_ms(self, key):
        ev = self.events.get(key, [])
        return (sum(s.elapsed_time(e) for s, e in ev) / len(ev)) if ev else None

    def mean_ms(self, key):
        ev = self.events.get(key, [])
        if not ev:
            return None, 0
        raw = sum(s.elapsed_time(e) for s, e in ev) / len(ev)
        return max(raw - 0.5 * getattr(self, "pair_ms", 0.0), 0.0), len(ev)


def cpu_model_name():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(cfg, state_dict, data, n_cascades, n_slices=1, ctx=None, ctx_name=""):
    """Time the oracle (CPU restatement of the reference path, torch CPU ops) on the same slice the GPU reconstructed, per BASELINE.md
    section 3: one untimed warm-up cascade, then `n_slices` slices of `n_cascades` cascades each, timed cascade by cascade (all cascades by
    default = whole slices; mean and min over the slices are reported), plus the FFT+DC step on its own.  Returns (cpu_baseline dict, the
    oracle's list[cascade][time_step] output of the first slice)."""
    import oracle
    ncores, box_cores = _oracle_threads()       # (the fastest thread count of the committed sweep, not os.cpu_count(): see there)
    T_ = oracle.models.cirim_time_steps(cfg["time_steps"])
    y, S, mask, target = data["y"], data["sensitivity_maps"], data["mask"], data["target"]
    import contextlib
    with torch.no_grad(), (ctx() if ctx is not None else contextlib.nullcontext()):     # (ctx: oracle.amp.autocast_fp16 for the precision-16 line)
        if ctx is None:         # (under autocast(float16) a cascade takes about a minute on the GPU box's host: no warm-up cascade there, its first-call costs are noise)
            oracle.models.cirim_forward(state_dict, dict(cfg, num_cascades=1), y, S, mask, None, target)       # warm-up, untimed
        stamps = [time.perf_counter()]
        ref = oracle.models.cirim_forward(state_dict, dict(cfg, num_cascades=n_cascades), y, S, mask, None, target,
                                          cascade_stamps=stamps)
        slice_s = [stamps[-1] - stamps[0]]
        for _ in range(max(n_slices, 1) - 1):                # further timed slices (the cost does not depend on the data: the same arrays again)
            t0 = time.perf_counter()
            oracle.models.cirim_forward(state_dict, dict(cfg, num_cascades=n_cascades), y, S, mask, None, target)
            slice_s.append(time.perf_counter() - t0)
        eta = torch.zeros(1, y.shape[2], y.shape[3], 2)
        oracle.rim.log_likelihood_gradient(eta, y, S, mask, 1.0, cfg["fft_centered"], cfg["fft_normalization"], cfg["spatial_dims"],
                                           cfg["coil_dim"])
        t0 = time.perf_counter()
        for _ in range(3):
            oracle.rim.log_likelihood_gradient(eta, y, S, mask, 1.0, cfg["fft_centered"], cfg["fft_normalization"],
                                               cfg["spatial_dims"], cfg["coil_dim"])
        llg_s = (time.perf_counter() - t0) / 3
    per = [b_ - a_ for a_, b_ in zip(stamps[:-1], stamps[1:])]
    dt = sum(per)
    sec_per_slice = (sum(slice_s) / len(slice_s)) * cfg["num_cascades"] / n_cascades
    step_s = dt / (n_cascades * T_)
    whole = n_cascades == cfg["num_cascades"]
    return dict(value=1.0 / sec_per_slice, unit="slices/s", cores=ncores, kind="port", box_cores=box_cores, cpu_model=cpu_model_name(),
                slices_timed=len(slice_s), sec_per_slice=[t * cfg["num_cascades"] / n_cascades for t in slice_s],
                sec_per_slice_mean=sec_per_slice, sec_per_slice_min=min(slice_s) * cfg["num_cascades"] / n_cascades,
                sec_per_cascade_mean=dt / n_cascades, sec_per_cascade_min=min(per), sec_per_cascade=per,
                split_ms_per_rim_step=dict(fft_dc=1e3 * llg_s, regulariser=1e3 * max(step_s - llg_s, 0.0)),
                sample=(("after one untimed warm-up cascade: " if ctx is None else "") + f"{len(slice_s)} slice(s) of {n_cascades} of {cfg['num_cascades']} cascades ({n_cascades * T_} of "
                        f"{cfg['num_cascades'] * T_} RIM steps) each on the oracle{ctx_name} (torch CPU ops, {ncores} threads of the box's "
                        f"{box_cores}), value = 1 / mean seconds per slice, {sum(slice_s):.1f} s in all"
                        + ("" if whole else f", extrapolated x{cfg['num_cascades'] / n_cascades:g}"))), ref


def parity_vs_oracle(gpu_pred, ref_pred, target, at):
    """The GPU reconstruction against the oracle's on the same weights and inputs: rel-L2 of the complex images and the metric's
    "SSIM vs ref" -- SSIM (harness formula, models/base.py:415-436) of the two `abs / max` images, computed by the PRODUCT
    (mridc_amd.runner on the device); the oracle's own SSIM of the same pair is the checker next to it."""
    import oracle
    from mridc_amd import runner
    got, want = gpu_pred.cpu(), ref_pred
    rel = float((torch.view_as_real(got).double() - torch.view_as_real(want).double()).norm() / torch.view_as_real(want).double().norm())
    dev = gpu_pred.device
    o_gpu, o_ref = runner.postprocess(gpu_pred, want.to(dev))                     # both through the product's post-processing
    m = runner.metrics_to_dict(runner.slice_metrics(o_gpu, o_ref))
    c1, _ = oracle.metrics.postprocess(got, want)
    c2, _ = oracle.metrics.postprocess(want, want)
    ssim_chk = oracle.metrics.ssim(c2.numpy(), c1.numpy(), maxval=float(c1.max() - c1.min()))
    vs_target = runner.metrics_to_dict(runner.slice_metrics(*runner.postprocess(gpu_pred, target.to(dev))))
    vs_target.pop("maxval")
    vs_target["note"] = "random-init weights (no checkpoint can be fetched here): quality against the ground truth is not meaningful"
    return dict(rel_l2=rel, ssim=m["SSIM"], ssim_oracle_check=ssim_chk, nmse=m["NMSE"], at=at, metrics_vs_target=vs_target)


_STREAM_POOL = []
_COPY_STREAM = []         # the upload stream of --stream-inputs: one per process, high priority (its own hardware queue)


def bench_streams(n):
    """The process's compute streams, created once and shared by every benchmark of the run: HIP maps streams onto a few hardware queues in
    creation order, and two FRESH streams created after a dozen others can land on one queue -- the in-process E2EVN line then read 820
    slices/s (its two slice batches serialised) against 1020 stand-alone."""
    prio = os.environ.get("MRX_BENCH_STREAM_PRIO")      # (A/B: "hi-lo" = the first compute stream at high priority: headline 152.8 against 152.2 slices/s, +0.4 %, not adopted -- tools/runs/r06ab.sh)
    while len(_STREAM_POOL) < n:
        _STREAM_POOL.append(torch.cuda.Stream(priority=-1 if (prio == "hi-lo" and not _STREAM_POOL) else 0))
    return _STREAM_POOL[:n]


def _tensors(o):
    """Every tensor of a nested output, in order."""
    if isinstance(o, torch.Tensor):
        return [o]
    if isinstance(o, (list, tuple)):
        return [t for e in o for t in _tensors(e)]
    return []


DUMP_LIMIT_BYTES = 64_000_000     # --dump-outputs: all files together, npy headers included
DUMP_SAMPLE_SEED = 0


def _named_leaves(o, name="out"):
    """(name, tensor) for every tensor of a nested output, named by its index path: CIRIM's list[cascade][time_step] -> out_<cascade>_<step>."""
    if isinstance(o, torch.Tensor):
        return [(name, o)]
    if isinstance(o, (list, tuple)):
        return [nt for i, e in enumerate(o) for nt in _named_leaves(e, f"{name}_{i}")]
    if isinstance(o, dict):
        return [nt for k, e in o.items() for nt in _named_leaves(e, f"{name}_{k}")]
    return []


def _dump_itemsize(t):
    return {torch.complex128: 16, torch.complex64: 8, torch.float64: 8}.get(t.dtype, 4)


def write_outputs(path, outs):
    """--dump-outputs: what the timed path returned in its last step.  `outs` = one nested output per stream (the same structure each); every
    leaf is written as path/<name>.npy with the streams stacked on a new leading axis, complex as a trailing (re, im) axis, in float64 if it is
    double precision and float32 otherwise.  If the whole set exceeds DUMP_LIMIT_BYTES, the LAST leaf (the final result) is written whole and
    every other leaf as the same number of elements at flat indices drawn once from a fixed seed, so that two runs with the same arguments
    write files that compare element for element."""
    import numpy as np
    leaves = [_named_leaves(o) for o in outs]
    names = [n for n, _ in leaves[0]]
    stacked = {n: [lv[j][1] for lv in leaves] for j, n in enumerate(names)}
    header = 256                                      # bytes per .npy header, generously
    numel = {n: sum(t.numel() for t in ts) for n, ts in stacked.items()}
    nbytes = {n: numel[n] * _dump_itemsize(ts[0]) for n, ts in stacked.items()}
    sample = None
    if sum(nbytes.values()) + header * len(names) > DUMP_LIMIT_BYTES:
        last, rest = names[-1], names[:-1]
        whole = nbytes[last] if nbytes[last] <= DUMP_LIMIT_BYTES // 2 else 0
        budget = DUMP_LIMIT_BYTES - whole - header * len(names)
        per = max(1, budget // max(1, len(rest) + (0 if whole else 1)) // 16)   # elements per sampled leaf (16 bytes: the widest element)
        sample = {n: per for n in (rest if whole else names)}
    os.makedirs(path, exist_ok=True)
    g = torch.Generator().manual_seed(DUMP_SAMPLE_SEED)
    written = 0
    for n in names:
        t = torch.stack([x.detach() for x in stacked[n]])
        if sample and n in sample:
            idx = torch.randint(0, t.numel(), (min(sample[n], t.numel()),), generator=g).sort().values
            t = t.reshape(-1)[idx.to(t.device)]
        if t.is_complex():
            t = torch.view_as_real(t)
        a = t.to(torch.float64 if t.dtype == torch.float64 else torch.float32).cpu().numpy()
        np.save(os.path.join(path, n + ".npy"), a)
        written += a.nbytes
    print(f"[bench] --dump-outputs: {len(names)} array(s), {written / 1e6:.1f} MB in {path}"
          + (f" (all but the last a seeded sample of {next(iter(sample.values()))} elements)" if sample else ""), file=sys.stderr)


def make_slices(C, H, W, indices, **kw):
    """synthetic.make_slice for every index, on a few host threads (numpy's FFTs release the GIL).  Every slice draws from its own seed, so the
    data do not depend on the number of threads."""
    from concurrent.futures import ThreadPoolExecutor
    from mridc_amd import synthetic
    indices = list(indices)
    n = max(1, min(16, len(indices), len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)))
    with ThreadPoolExecutor(max_workers=n) as ex:
        return list(ex.map(lambda i: synthetic.make_slice(C, H, W, slice_idx=i, **kw), indices))


LAST_CONCURRENCY_CHECK = {}


def concurrent_replays_match_serial(graphs, streams, outs):
    """After the timed (concurrent) replays: replay every graph once more ALONE and compare its outputs, bit for bit, with what the concurrent
    replays left there -- kernels of different slices sharing CUs must not influence each other ("Concurrent streams").  None
    without graphs or with a single stream."""
    if not graphs or len(graphs) < 2:
        return None
    torch.cuda.synchronize()
    conc = [[t.clone() for t in _tensors(o)] for o in outs]
    for g_, st in zip(graphs, streams):
        with torch.cuda.stream(st):
            g_.replay()
        torch.cuda.synchronize()
    return all(torch.equal(a, b) for c, o in zip(conc, outs) for a, b in zip(c, _tensors(o)))


def _replay_loop(step, datas, args):
    """Shared timed region of the inference benchmarks: one HIP stream + one captured hipGraph per in-flight slice batch, args.steps
    replays each, barrier + synchronize on both sides, max over ranks.  Returns (elapsed, per_rank, graphed, last outputs)."""
    NS = len(datas)
    streams = bench_streams(NS)
    graphs, outs = [], [None] * NS
    if args.graph:
        try:
            for i, (d, st) in enumerate(zip(datas, streams)):
                st.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(st):
                    step(d)
                torch.cuda.current_stream().wait_stream(st)
                g_ = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g_, stream=st, capture_error_mode="thread_local"):
                    outs[i] = step(d)
                graphs.append(g_)
            for g_, st in zip(graphs, streams):          # one untimed replay each (as the headline loop does): the first launch of a graph
                with torch.cuda.stream(st):              # uploads it -- ~10 ms when other graphs already live in the process
                    g_.replay()
            torch.cuda.synchronize()
        except Exception as ex:  # noqa: BLE001
            print(f"[bench] hipGraph capture unavailable ({type(ex).__name__}: {ex}); timing eager launches", file=sys.stderr)
            graphs = []
            torch.cuda.synchronize()
    dist_barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        for i, st in enumerate(streams):
            with torch.cuda.stream(st):
                if graphs:
                    graphs[i].replay()
                else:
                    outs[i] = step(datas[i])
    dist_barrier()
    elapsed, per_rank = rank_times(time.perf_counter() - t0, torch.device("cuda", torch.cuda.current_device()))
    if args.dump_outputs and int(os.environ.get("RANK", "0")) == 0:
        write_outputs(args.dump_outputs, outs)
    LAST_CONCURRENCY_CHECK["bit_identical"] = concurrent_replays_match_serial(graphs, streams, outs) if args.full else None
    return elapsed, per_rank, bool(graphs), outs


def _event_profile(timer, step, d, n=2):
    """`n` eager steps with the timer's HIP events on (host enqueues ahead of a parked GPU), then the empty-pair calibration."""
    timer.enabled = True
    torch.cuda.synchronize()
    try:
        torch.cuda._sleep(int(4e7))
    except Exception:  # noqa: BLE001
        pass
    for _ in range(n):
        step(d)
    timer.calibrate()
    timer.enabled = False


ORACLE_THREADS_DEFAULT = 16       # the best of the committed sweep (profiles/r05_cpu_thread_sweep.txt: 8 / 16 / 32 / 64 / 128 / 256 threads on the GPU box's 256-thread host, stand-alone and inside this bench)


def _oracle_threads():
    """Threads for the CPU oracle: BASELINE.md section 3 says os.cpu_count(); on the GPU box's 256-thread host these op sizes run several times
    SLOWER with every thread than with 32 (tools/probe/cpu_thread_sweep.py, committed under profiles/), so the baseline uses the fastest setting
    of that sweep -- the one that flatters the CPU most.  MRX_ORACLE_THREADS overrides it."""
    box_cores = os.cpu_count() or 1
    want = int(os.environ.get("MRX_ORACLE_THREADS", "0")) or ORACLE_THREADS_DEFAULT
    ncores = max(1, min(box_cores, want))
    torch.set_num_threads(ncores)
    return ncores, box_cores


QCIRIM_CFG = {"quantitative_module_recurrent_layer": "IndRNN", "quantitative_module_conv_filters": [128, 128, 4],
              "quantitative_module_conv_kernels": [5, 3, 3], "quantitative_module_conv_dilations": [1, 2, 1],
              "quantitative_module_conv_bias": [True, True, False], "quantitative_module_recurrent_filters": [128, 128, 0],
              "quantitative_module_recurrent_kernels": [1, 1, 0], "quantitative_module_recurrent_dilations": [1, 1, 0],
              "quantitative_module_recurrent_bias": [True, True, False], "quantitative_module_depth": 2,
              "quantitative_module_time_steps": 8, "quantitative_module_num_cascades": 1, "quantitative_module_no_dc": True,
              "quantitative_module_signal_forward_model_sequence": "MEGRE", "quantitative_module_dimensionality": 2,
              "quantitative_module_gamma_regularization_factors": [150.0, 150.0, 1000.0, 150.0], "use_reconstruction_module": False,
              "fft_centered": False, "fft_normalization": "backward", "spatial_dims": [-2, -1], "coil_dim": 2,
              "coil_combination_method": "SENSE"}


def bench_qcirim(args, world, rank, dev, checks=False):
    """configs[4]: qCIRIM (quantitative R2*/S0/B0/phi mapping), 4 echoes, 32 coils, 256x256, IndRNN 128 filters, 1 cascade x 8 time-steps
    (projects/quantitative/model_zoo/conf/base_qcirim_run.yaml defaults; quantitative/models/qcirim.py:144-312).
    `checks`: HIP-event roofline of the dominant kernel, the oracle timed on the host (cpu_baseline) and parity of the final maps."""
    from mridc_amd import ops
    from mridc_amd.collections.quantitative.models.qcirim import qCIRIM
    cfg = QCIRIM_CFG
    p16 = args.precision == 16          # the reference's own inference precision (base_qcirim_run.yaml:204): the 128 -> 128 3x3 convolutions on one fp16 term
    torch.manual_seed(0)
    model = qCIRIM(dict(cfg, precision=16) if p16 else cfg).eval()
    state_dict = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(dev)
    E, C, H, W = 4, 32, 256, 256
    TEs = [3.0, 11.5, 20.0, 28.5]
    NS = max(1, args.streams)
    hosts, datas = [], []
    for i in range(NS):
        g = torch.Generator().manual_seed(100 + rank * NS + i)
        maps = [torch.rand(1, H, W, generator=g) * s for s in (0.3, 1.0, 0.1, 0.5)]
        S = torch.randn(1, C, H, W, 2, generator=g) / C ** 0.5
        mask = (torch.rand(1, 1, 1, 1, W, 1, generator=g) < 0.3)
        y = torch.randn(1, E, C, H, W, 2, generator=g) * mask
        hosts.append(maps + [y, S, mask])
        datas.append([t.to(dev) for t in hosts[-1]])

    def step(d):
        with torch.no_grad():
            return next(model(d[0], d[1], d[2], d[3], TEs, d[4], d[5], None, d[6]))

    timer = KernelTimer()
    if checks:
        timer.wrap(ops, "conv3x3_wino", lambda x, w, *a, **k: "wino_%dx%d" % (int(w.shape[1]), int(w.shape[0])))
        timer.wrap(ops, "conv3x3_h", lambda x, w, *a, **k: "h3x3_%dx%d" % (int(w.shape[1]), int(w.shape[0])))
    for _ in range(max(args.warmup, 1)):
        step(datas[0])
    torch.cuda.synchronize()
    if checks:
        _event_profile(timer, step, datas[0])
    elapsed, per_rank, graphed, outs = _replay_loop(step, datas, args)
    conc_ok = LAST_CONCURRENCY_CHECK.get("bit_identical")
    res = dict(metric="slices/sec (inference), qCIRIM 4-echo 32-coil 256x256" + (", precision 16" if p16 else ""), value=world * NS * args.steps / elapsed,
               unit="slices/s", n_gpus=world, steps=args.steps, warmup=args.warmup, ms_per_step=1e3 * elapsed / args.steps,
               higher_is_better=True, scaling="weak", vs_baseline=None, world_size_seen=world_seen(),
               per_rank_ms_per_step=[1e3 * t / args.steps for t in per_rank],
               dtype="f16 operands in the 128 -> 128 3x3 convolutions (fp32 sums; 5x5 / 1x1 layers, signal model, FFT fp32-class)" if p16 else "f32", data="synthetic",
               config=dict(workload=f"qCIRIM 1 cascade x 8 time-steps, IndRNN 128 filters, 4 echoes, 32 coils, 256x256, {NS} slice(s) "
                                    f"per GPU and step ({NS} HIP stream(s), {'hipGraph' if graphed else 'eager'}), random-init weights" + (", trainer.precision = 16" if p16 else ""),
                           parallelism=f"slice-sharded x{world}"))
    if args.full:
        res["concurrent_replays_bit_identical_to_serial"] = conc_ok
    if checks and rank == 0:
        direct = 2.0 * 128 * 128 * 9 * H * W
        msh, nh = timer.mean_ms("h3x3_128x128")
        if msh:
            # the default: the 128 -> 128 3x3 dilation-2 layer on two-term fp16 operands (mrx_conv3x3_h): 3 term products per multiply, the 18 tap
            # slots of a 16-channel step padded to 20 (five MFMAs of four slots)
            issued = direct * (1.0 if p16 else 3.0) * 20.0 / 18.0
            res["roofline"] = dict(
                bound="mfma", kernel=f"k_uconv_h<4, 2, false> via mrx_conv3x3_{'p16' if p16 else 'h'} (the qRIM's 3x3 dilation-2 128 -> 128 convolution: {'one-term' if p16 else 'two-term'} fp16 operands on "
                                     f"v_mfma_f32_16x16x32_f16, {1 if p16 else 3} term product(s), fp32 accumulation; 4 cout blocks of 16 per work item; the bound of its input "
                                     "kept by the preceding 1x1 cell kernel)",
                achieved=issued / (msh * 1e-3) / 1e12, peak=PEAK_BF16_MFMA_TFLOPS, unit="TFLOP/s", frac=issued / (msh * 1e-3) / 1e12 / PEAK_BF16_MFMA_TFLOPS,
                frac_meaning="fp16 MFMA FLOPs the kernel issues (3 term products, slot padding included) / dense fp16 MFMA peak",
                algorithmic_achieved=direct / (msh * 1e-3) / 1e12, launches=nh, avg_ms=msh, flops_per_launch=direct, mfma_flops_per_launch=issued,
                traffic=measured_traffic(1, 15, 640, 372, 64).get("qcirim_conv3x3_h_128") if ((H, W) == (256, 256) and not p16) else None, traffic_unit="bytes/launch",
                mfma_util_pmc=(measured_traffic(1, 15, 640, 372, 64).get("_mfma_util") or {}).get("qcirim_conv3x3_h_128") if ((H, W) == (256, 256) and not p16) else None,
                algorithmic_bytes=2.0 * 128 * H * W * 4, hbm_frac=2.0 * 128 * H * W * 4 / (msh * 1e-3) / 1e9 / PEAK_HBM_GBS)
        else:
            ms, n = timer.mean_ms("wino_128x128")
            issued = direct * 4.0 / 9.0                     # Winograd F(2x2,3x3): 16 instead of 36 multiplies per 2x2 outputs
            res["roofline"] = dict(
                bound="mfma", kernel="k_rim_layer_wino<DIL 2, no tail> via mrx_conv3x3_wino (the qRIM's 3x3 dilation-2 128 -> 128 convolution as Winograd "
                                     "F(2x2,3x3) on fp32 MFMAs, two 64-cout blocks)",
                achieved=(issued / (ms * 1e-3) / 1e12) if ms else None, peak=PEAK_FP32_MFMA_TFLOPS, unit="TFLOP/s",
                frac=(issued / (ms * 1e-3) / 1e12 / PEAK_FP32_MFMA_TFLOPS) if ms else None,
                frac_meaning="MFMA FLOPs the kernel issues / fp32-MFMA peak", algorithmic_achieved=(direct / (ms * 1e-3) / 1e12) if ms else None,
                launches=n, avg_ms=ms, flops_per_launch=direct, mfma_flops_per_launch=issued, traffic=None,
                algorithmic_bytes=2.0 * 128 * H * W * 4)
        try:
            import oracle
            ncores, box_cores = _oracle_threads()
            h = hosts[0]
            # (precision 16: torch's CPU autocast needs 300 s per slice at this size -- 128-channel fp16 convolutions -- so the fp32 oracle is timed and compared
            # here; the autocast checker runs at 8 coils x 64 x 64 in tests/test_gpu_unet_p16.py)
            with torch.no_grad():
                oracle.qrim.qcirim_forward(state_dict, cfg, h[0], h[1], h[2], h[3], TEs, h[4], h[5], None, h[6])          # warm-up
                dts = []
                for _ in range(max(1, args.cpu_slices)):
                    t0 = time.perf_counter()
                    ref = oracle.qrim.qcirim_forward(state_dict, cfg, h[0], h[1], h[2], h[3], TEs, h[4], h[5], None, h[6])
                    dts.append(time.perf_counter() - t0)
                dt = sum(dts) / len(dts)
            res["cpu_baseline"] = dict(value=1.0 / dt, unit="slices/s", cores=ncores, kind="port", box_cores=box_cores, cpu_model=cpu_model_name(),
                                       slices_timed=len(dts), sec_per_slice=dts,
                                       sample=f"{len(dts)} whole slice(s) (1 cascade x 8 time-steps) on the {'fp32 ' if p16 else ''}oracle after one untimed warm-up slice, "
                                              f"torch CPU ops on {ncores} threads, value = 1 / mean seconds per slice, {sum(dts):.1f} s in all")
            out = outs[0] if graphed else step(datas[0])
            torch.cuda.synchronize()
            rels = []
            for m_ in range(4):                          # the four final maps (R2*, S0, B0, phi): last cascade, last time-step
                got, want = out[1 + m_][-1][-1].cpu().double(), ref[1 + m_][-1][-1].double()
                rels.append(float((got - want).norm() / want.norm()))
            res["parity_vs_oracle"] = dict(rel_l2=max(rels), rel_l2_per_map=dict(zip(("R2star", "S0", "B0", "phi"), rels)),
                                           at="the four maps after the last time-step, same weights and inputs"
                                              + ("; checker: the fp32 oracle (the reference's autocast arithmetic costs 300 s per slice on this host: tests/test_gpu_unet_p16.py "
                                                 "checks against it at 8 coils x 64 x 64), tolerance 3e-2" if p16 else ""))
        except Exception as ex:  # noqa: BLE001
            res["cpu_baseline"] = dict(value=None, unit="slices/s", cores=os.cpu_count(), kind="port", sample=f"failed: {type(ex).__name__}: {ex}")
    return res


def bench_e2evn(args, world, rank, dev, checks=False):
    """configs[1]: E2EVN 6 cascades, NormUnet(14, 2, pad 11), 15 coils 640x372 (reported next to the headline number)."""
    from mridc_amd import synthetic
    from mridc_amd.sharding import shard_range
    common = dict(fft_centered=False, fft_normalization="backward", spatial_dims=[-2, -1], coil_dim=1, coil_combination_method="SENSE",
                  use_sens_net=False)
    torch.manual_seed(0)
    if args.model == "e2evn":
        from mridc_amd.collections.reconstruction.models.vn import VarNet
        ucfg = dict(synthetic.E2EVN_BASELINE_CFG)
        if args.unet == "18x4":
            ucfg.update(channels=18, pooling_layers=4, padding_size=15)
        p16 = args.precision == 16          # the reference's own inference precision (base_vn_run.yaml:98): one-term fp16 3x3 convolutions, the rest fp32
        model = VarNet(dict(ucfg, precision=16) if p16 else ucfg)
        label = "E2EVN 6-cascade" + ("" if args.unet == "14x2" else " (NormUnet 18x4)") + (", precision 16" if p16 else "")
        desc = f"E2EVN 6 cascades, NormUnet(chans {ucfg['channels']}, pools {ucfg['pooling_layers']}, pad {ucfg['padding_size']})" + (", trainer.precision = 16" if p16 else "")
    elif args.model == "rvn":       # SURVEY 8f N4; the reference's base_rvn_run.yaml
        from mridc_amd.collections.reconstruction.models.rvn import RecurrentVarNet
        model = RecurrentVarNet(dict(common, in_channels=2, recurrent_hidden_channels=64, recurrent_num_layers=4, num_steps=8,
                                     no_parameter_sharing=True, learned_initializer=True, initializer_initialization="sense",
                                     initializer_channels=[32, 32, 64, 64], initializer_dilations=[1, 1, 2, 4], initializer_multiscale=1))
        label, desc = "RecurrentVarNet 8-step", "RecurrentVarNet 8 steps x 4 Conv2dGRU layers (64 features), learned initializer"
    elif args.model == "ccnn":      # base_ccnn_run.yaml
        from mridc_amd.collections.reconstruction.models.ccnn import CascadeNet
        model = CascadeNet(dict(common, num_cascades=10, hidden_channels=64, n_convs=5, batchnorm=False, no_dc=True))
        label, desc = "CascadeNet 10-cascade", "CascadeNet 10 cascades x 5 convs (64 channels), no_dc as in the model zoo"
    else:                           # base_vsnet_run.yaml
        from mridc_amd.collections.reconstruction.models.vsnet import VSNet
        model = VSNet(dict(common, num_cascades=10, imspace_model_architecture="CONV", imspace_conv_hidden_channels=64,
                           imspace_conv_n_convs=4, imspace_conv_batchnorm=False))
        label, desc = "VSNet 10-cascade", "VSNet 10 cascades, CONV denoiser (4 convs, 64 channels, shared)"
    model = model.eval()
    state_dict = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(dev)
    B, C, H, W = args.batch, args.coils, args.height, args.width
    NS = max(1, args.streams)
    s0, s1 = shard_range(world * NS * B, rank, world)
    datas, hosts = [], []
    for i in range(NS):
        slices = make_slices(C, H, W, range(s0 + i * B, s0 + (i + 1) * B), mask_dtype=torch.float32 if args.model == "vsnet" else torch.uint8)
        h_ = {k: torch.cat([s[k] for s in slices], 0) for k in ("y", "sensitivity_maps", "target")}
        h_["mask"] = slices[0]["mask"]
        hosts.append(h_)
        datas.append({k: v.to(dev) for k, v in h_.items()})

    def step(d):
        with torch.no_grad():
            return model(d["y"], d["sensitivity_maps"], d["mask"], None, d["target"])

    checks = checks and args.model == "e2evn"
    timer = KernelTimer()
    if checks:
        from mridc_amd import ops
        timer.wrap(ops, "unet_conv3x3", lambda a_, b_, w, *r, **k: "uconv %d->%d @%dx%d" % (
            int(w.shape[1]), int(w.shape[0]), int((a_[0] if isinstance(a_, tuple) else a_).shape[2]), int((a_[0] if isinstance(a_, tuple) else a_).shape[3])))
    for _ in range(max(args.warmup, 1)):
        step(datas[0])
    torch.cuda.synchronize()
    if checks:
        _event_profile(timer, step, datas[0])
    elapsed, per_rank, graphed, outs = _replay_loop(step, datas, args)
    conc_ok = LAST_CONCURRENCY_CHECK.get("bit_identical")
    Bt = NS * B
    res = dict(metric=f"slices/sec (inference), {label} {C}-coil {H}x{W}", value=world * Bt * args.steps / elapsed,
               unit="slices/s", n_gpus=world, steps=args.steps, warmup=args.warmup,
               ms_per_step=1e3 * elapsed / args.steps, higher_is_better=True, scaling="weak", vs_baseline=None, world_size_seen=world_seen(),
               per_rank_ms_per_step=[1e3 * t / args.steps for t in per_rank],
               dtype="f16 operands in the U-Net's 3x3 convolutions (fp32 sums, fp32 activations / statistics / FFT / data consistency)" if (args.model == "e2evn" and args.precision == 16) else "f32",
               data="synthetic",
               config=dict(workload=f"{desc}, {C} coils, {H}x{W}, batch "
                                    f"{Bt} per GPU ({NS} concurrent HIP stream(s), {'one hipGraph each' if graphed else 'eager'}), random-init weights "
                                    "(seed 0)", parallelism=f"slice-sharded x{world}"))
    if args.full:
        res["concurrent_replays_bit_identical_to_serial"] = conc_ok
    if checks and rank == 0:
        # dominant kernel: the U-Net's 3x3 convolutions (k_uconv: fp32 MFMA 16x16x4 blocks, InstanceNorm statistics from the accumulators,
        # normalisation + LeakyReLU of the PREVIOUS layer applied by the tile loader) -- the shape that takes the most time
        tot = {k: sum(s_.elapsed_time(e_) for s_, e_ in v) for k, v in timer.events.items()}
        if tot:
            key = max(tot, key=tot.get)
            ms, n = timer.mean_ms(key)
            cin, rest = key.split(" ")[1].split("->")[0], key.split("->")[1]
            cout, hw = rest.split(" @")
            hh_, ww_ = (int(v) for v in hw.split("x"))
            flops = 2.0 * int(cin) * int(cout) * 9 * hh_ * ww_ * B
            all_ms = sum(tot.values()) / 2.0                    # two profiled steps (raw event time of every U-Net 3x3 convolution)
            from mridc_amd import _lib as _l
            nbytes = (int(cin) + int(cout)) * hh_ * ww_ * B * 4.0
            terms = 1 if args.precision == 16 else 3
            if ops.UNET_F16 and _l.arith() == "f16x2":
                # the default: two-term fp16 operands -- the matrix work is 3 / 16 of the fp32-input form's cycles and the launch is bound by its
                # tile loads and stores (algorithmic bytes = every input plane read once + every output plane written once)
                gbs = (nbytes / (ms * 1e-3) / 1e9) if ms else None
                res["roofline"] = dict(bound="hbm", kernel=f"k_uconv_h via mrx_unet_conv3x3_{'p16' if terms == 1 else 'h'} ({key}: 3x3 zero-padded convolution, batch {B}, {'one-term' if terms == 1 else 'two-term'} fp16 operands "
                                                              f"on v_mfma_f32_16x16x32_f16 ({terms} term product(s), fp32 accumulation), fused InstanceNorm statistics; the previous "
                                                              "layer's normalisation + LeakyReLU and the operand split in the tile loader)",
                                       achieved=gbs, peak=PEAK_HBM_GBS, unit="GB/s", frac=(gbs / PEAK_HBM_GBS) if gbs else None,
                                       frac_meaning="algorithmic bytes of the launch (inputs read once + outputs written once) / 8 TB/s", launches=n, avg_ms=ms,
                                       # counter traffic exists for the 14 -> 14 layer at 4 x 640 x 380 (tools/probe/pmc_r04.py) and at the default line's
                                       # 8 x 640 x 380 (pmc_r04_b8.py): the shape this record names by default
                                       traffic=(measured_traffic(8 if B == 8 else 1, 15, 640, 372, 64).get("e2evn_uconv_h_14to14")
                                                if (int(cin), int(cout), hh_, ww_) == (14, 14, 640, 380) and B in (4, 8) and terms == 3 else None),
                                       traffic_unit="bytes/launch",
                                       mfma_util_pmc=((measured_traffic(8 if B == 8 else 1, 15, 640, 372, 64).get("_mfma_util") or {}).get("e2evn_uconv_h_14to14")
                                                      if (int(cin), int(cout), hh_, ww_) == (14, 14, 640, 380) and B in (4, 8) and terms == 3 else None),
                                       algorithmic_bytes=nbytes, flops_per_launch=flops,
                                       mfma_frac=(terms * flops / (ms * 1e-3) / 1e12 / PEAK_BF16_MFMA_TFLOPS) if ms else None,
                                       all_unet_conv3x3_ms_per_step=all_ms)
            else:
                res["roofline"] = dict(bound="mfma", kernel=f"k_uconv via mrx_unet_conv3x3 ({key}: 3x3 zero-padded convolution, batch {B}, fp32 MFMA 16x16x4, fused "
                                                              "InstanceNorm statistics; the previous layer's normalisation + LeakyReLU in the tile loader)",
                                       achieved=(flops / (ms * 1e-3) / 1e12) if ms else None, peak=PEAK_FP32_MFMA_TFLOPS, unit="TFLOP/s",
                                       frac=(flops / (ms * 1e-3) / 1e12 / PEAK_FP32_MFMA_TFLOPS) if ms else None,
                                       frac_meaning="direct-form MFMA FLOPs of the launch / fp32-MFMA peak", launches=n, avg_ms=ms, flops_per_launch=flops,
                                       traffic=None, algorithmic_bytes=nbytes,
                                       hbm_frac=(nbytes / (ms * 1e-3) / 1e9 / PEAK_HBM_GBS) if ms else None,
                                       all_unet_conv3x3_ms_per_step=all_ms)
        try:
            import oracle
            ncores, box_cores = _oracle_threads()
            h1 = {k: (v[:1] if k != "mask" else v) for k, v in hosts[0].items()}
            # (precision 16: the reference's own arithmetic on the CPU -- torch.autocast(float16), oracle/amp.py -- is both the baseline that is timed and the checker)
            import contextlib
            with torch.no_grad(), (oracle.amp.autocast_fp16() if args.precision == 16 else contextlib.nullcontext()):
                oracle.models.varnet_forward(state_dict, dict(ucfg, num_cascades=1), h1["y"], h1["sensitivity_maps"], h1["mask"], None, h1["target"])
                dts = []
                for _ in range(max(1, args.cpu_slices)):
                    t0 = time.perf_counter()
                    ref = oracle.models.varnet_forward(state_dict, ucfg, h1["y"], h1["sensitivity_maps"], h1["mask"], None, h1["target"])
                    dts.append(time.perf_counter() - t0)
                dt = sum(dts) / len(dts)
            res["cpu_baseline"] = dict(value=1.0 / dt, unit="slices/s", cores=ncores, kind="port", box_cores=box_cores, cpu_model=cpu_model_name(),
                                       slices_timed=len(dts), sec_per_slice=dts,
                                       sample=f"{len(dts)} whole slice(s) ({ucfg['num_cascades']} cascades) on the oracle{' under torch.autocast(float16)' if args.precision == 16 else ''} after one untimed warm-up cascade, torch CPU "
                                              f"ops on {ncores} threads, value = 1 / mean seconds per slice, {sum(dts):.1f} s in all")
            out = outs[0] if graphed else step(datas[0])
            torch.cuda.synchronize()
            res["parity_vs_oracle"] = parity_vs_oracle(out[0:1], ref[0:1].to(torch.complex64), h1["target"], at="the final image (all cascades, SENSE combination)"
                                                       + ("; checker: the oracle under torch.autocast(float16), tolerance 3e-2 (SURVEY appendix C)" if args.precision == 16 else ""))
            if args.precision == 16:
                with torch.no_grad():
                    ref32 = oracle.models.varnet_forward(state_dict, ucfg, h1["y"], h1["sensitivity_maps"], h1["mask"], None, h1["target"])
                res["parity_vs_fp32_oracle"] = parity_vs_oracle(out[0:1], ref32[0:1], h1["target"], at="the final image against the fp32 oracle")
                res["autocast_oracle_vs_fp32_oracle"] = parity_vs_oracle(ref[0:1].to(torch.complex64).to(out.device), ref32[0:1], h1["target"], at="the reference's own precision-16 arithmetic against fp32")
        except Exception as ex:  # noqa: BLE001
            res["cpu_baseline"] = dict(value=None, unit="slices/s", cores=os.cpu_count(), kind="port", sample=f"failed: {type(ex).__name__}: {ex}")
    return res


def bench_train(args, world, rank, dev, checks=False):
    """BASELINE config C4 (CIRIM training, DDP gradient all-reduce): one slice per rank and step, fp32."""
    from mridc_amd import autograd as ag
    from mridc_amd import synthetic, training
    from mridc_amd.collections.reconstruction.models.cirim import CIRIM
    ag.set_precision(args.dtype)       # bf16: convolution / IndRNN GEMM operands in bf16, fp32 accumulation, forward and backward
    cfg = dict(synthetic.CIRIM_BASELINE_CFG)
    cfg["recurrent_layer"] = "IndRNN"
    if args.cascades:
        cfg["num_cascades"] = args.cascades
    torch.manual_seed(0)
    C, H, W = args.coils, args.height, args.width
    s = synthetic.make_slice(C, H, W, slice_idx=rank)
    batch = {k: s[k].to(dev) for k in ("y", "sensitivity_maps", "mask", "target")}
    if args.model == "e2evn":           # E2EVN under the same trainer (vn.py): forward recorded through mridc_amd.diff
        from mridc_amd.collections.reconstruction.models.vn import VarNet
        ucfg = dict(synthetic.E2EVN_BASELINE_CFG)
        if args.unet == "18x4":
            ucfg.update(channels=18, pooling_layers=4, padding_size=15)
        model = VarNet(ucfg).to(dev)
        step_fn = training.model_training_step
    else:
        model = CIRIM(cfg).to(dev)
        step_fn = training.training_step
    flat = training.FlatParameters(model)
    opt = training.AdamFlat(flat, lr=1e-3, betas=(0.9, 0.98))
    graphed = None
    checks = checks and args.model != "e2evn" and rank == 0
    timer = KernelTimer()
    if checks:
        from mridc_amd import ops
        timer.wrap(ops, "conv2d_bf16", lambda x, w, b_, dil=1, *a_, **k: "conv_bf16 %dx%d %d->%d d%d%s" % (
            int(w.shape[2]), int(w.shape[3]), int(w.shape[0] if k.get("transposed") else w.shape[1]),
            int(w.shape[1] if k.get("transposed") else w.shape[0]), int(dil), " (data gradient)" if k.get("transposed") else ""))
        # the bf16-storage tape (round 4)
        timer.wrap(ops, "tl_cell_bwd", lambda *a_, **k: "tl_cell_bwd")
        timer.wrap(ops, "tl_layer_fwd", lambda x, *a_, **k: "tl_layer_fwd %d->64" % int(x.shape[1]))
        timer.wrap(ops, "conv_wgrad_bf16_pairs", lambda x, dy, kk, *a_, **k: "wgrad from pairs %dx%d %d->64" % (int(kk), int(kk), int(x.shape[1])))
        timer.wrap(ops, "tl_dgrad", lambda dy, w, *a_, **k: "tl_dgrad %d->%d (+ edge fold)" % (int(w.shape[0]), int(w.shape[1])))
    losses = []
    if args.model != "e2evn" and args.train_graph:
        try:
            graphed = training.GraphedCirimStep(model, flat, opt, batch)
            step_fn = lambda m_, f_, o_, b_: graphed(b_)       # noqa: E731
        except Exception as ex:  # noqa: BLE001
            print(f"[bench] training-step capture failed ({type(ex).__name__}: {ex}); eager step", file=sys.stderr)
            graphed = None
    if args.model == "e2evn" and args.graph:
        # forward + loss + backward as ONE hipGraph replay (a few thousand short launches: issued from Python the step is host-bound and jitters);
        # all-reduce and Adam outside.  Falls back to the eager step if the capture fails.
        try:
            graphed = training.GraphedModelStep(model, flat, opt, batch)
            step_fn = lambda m_, f_, o_, b_: graphed(b_)       # noqa: E731
        except Exception as ex:  # noqa: BLE001
            print(f"[bench] training-step capture failed ({type(ex).__name__}: {ex}); eager step", file=sys.stderr)
            graphed = None
    for _ in range(max(args.warmup, 1)):
        losses.append(float(step_fn(model, flat, opt, batch)))
    if checks:
        keep_side = training.TL_SIDE_STREAM
        training.TL_SIDE_STREAM = False                  # the profiled step serially: a kernel's events must not contain a neighbour from the side stream
        try:
            _event_profile(timer, lambda d: training.training_step(model, flat, opt, d), batch, n=1)      # (eager also when the timed steps are graph replays)
        finally:
            training.TL_SIDE_STREAM = keep_side
        step_fn(model, flat, opt, batch)                 # untimed: back to the two-stream form (the serial profiled step left the side stream's pool cold)
    dist_barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step_fn(model, flat, opt, batch)
    dist_barrier()
    elapsed, per_rank = rank_times(time.perf_counter() - t0, dev)
    if args.dump_outputs and rank == 0:            # what a caller of the step has afterwards: the step's loss and the updated parameters
        write_outputs(args.dump_outputs, [dict(loss=torch.as_tensor(loss).reshape(1), parameters=flat.flat)])
    losses.append(float(loss))
    if args.model == "e2evn":
        return dict(metric=f"slices/sec (training), E2EVN {ucfg['num_cascades']}-cascade {C}-coil {H}x{W}", value=world * args.steps / elapsed,
                    unit="slices/s", n_gpus=world, steps=args.steps, warmup=args.warmup, ms_per_step=1e3 * elapsed / args.steps,
                    higher_is_better=True, scaling="weak", vs_baseline=None, world_size_seen=world_seen(),
                    per_rank_ms_per_step=[1e3 * t / args.steps for t in per_rank], dtype="f32", data="synthetic",
                    config=dict(workload=f"E2EVN {ucfg['num_cascades']} cascades, NormUnet({ucfg['channels']}, {ucfg['pooling_layers']}), {C} coils, "
                                         f"{H}x{W}: forward + l1 loss + backward (convolution / transposed-convolution / FFT gradients on the HIP "
                                         f"kernels, coil operators / data consistency / activation / InstanceNorm / pooling backward on csrc/diff_bwd.hip) + one all-reduce of the flat "
                                         f"gradient ({flat.numel * 4 / 1e6:.2f} MB) + Adam, 1 slice per GPU and step",
                                launch=("forward + loss + backward = one hipGraph replay (training.GraphedModelStep; weight packs inside the graph), "
                                        "all-reduce + Adam eager") if graphed is not None else "eager",
                                global_batch=world, parallelism=f"data-parallel x{world}", gradient_bytes=flat.numel * 4),
                    loss_first=losses[0], loss_last=losses[-1])
    res = dict(metric=f"slices/sec (training), CIRIM {cfg['num_cascades']}-cascade {C}-coil {H}x{W}",
               value=world * args.steps / elapsed, unit="slices/s", n_gpus=world, steps=args.steps, warmup=args.warmup,
               ms_per_step=1e3 * elapsed / args.steps, higher_is_better=True, scaling="weak", vs_baseline=None, world_size_seen=world_seen(),
               per_rank_ms_per_step=[1e3 * t / args.steps for t in per_rank],
               dtype=args.dtype, data="synthetic",
               config=dict(workload=f"CIRIM {cfg['num_cascades']} cascades x {model.time_steps} time-steps, IndRNN 64, {C} coils, "
                                    f"{H}x{W}: forward + l1 loss + backward (HIP kernels) + one all-reduce of the flat gradient "
                                    f"({flat.numel * 4 / 1e6:.2f} MB) + Adam, 1 slice per GPU and step"
                                    + ("; convolutions and IndRNN GEMMs on bf16 operands with fp32 accumulation (forward, data and "
                                       "weight gradients), their results -- and the gradients flowing into them -- STORED in bf16 (the rounding points of "
                                       "torch.autocast: what the reference's `precision: 16` does), hidden states / FFT / data consistency / eta / loss / "
                                       "parameter-gradient sums / Adam in fp32; weight gradients on a second HIP stream" if args.dtype == "bf16"
                                       else ""),
                           global_batch=world, parallelism=f"data-parallel x{world}", gradient_bytes=flat.numel * 4),
               loss_first=losses[0], loss_last=losses[-1])
    if checks:
        tot = {k: sum(s_.elapsed_time(e_) for s_, e_ in v) for k, v in timer.events.items()}
        if tot:
            key = max(tot, key=tot.get)
            ms, n = timer.mean_ms(key)
            share = {k: v / 1.0 for k, v in sorted(tot.items(), key=lambda kv: -kv[1])[:6]}
            table = measured_traffic(1, 15, 640, 372, 64) if (C, H, W) == (15, 640, 372) else {}
            if key == "tl_cell_bwd":
                # bytes of one launch: dh_above (pairs, 2 B) + dH + h_prev (fp32) + a (pairs) read, dh_prev (fp32) + ga (pairs) written, 64 channels;
                # the layer's own state as its (h > 0) mask words, 8 bytes per pixel
                nbytes = ((2 + 4 + 4 + 2 + 4 + 2) * 64.0 + 8.0) * H * W
                res["roofline"] = dict(bound="hbm", kernel="k_tl_cell_bwd via mrx_tl_cell_bwd: the backward of an IndRNN layer's cell and of its convolution's ReLU in one pass -- "
                                                            "g = (dh_above + dH) (h > 0), dh_prev, the hh / bias sums, da = bf16(W_ih^T bf16(g)) and dW_ih += bf16(g) a^T on "
                                                            "v_mfma_f32_32x32x16_bf16, ga = da (a > 0) as a pair tensor (replaces five launches of the fp32-storage tape); the kernel "
                                                            "with the largest share of a training step",
                                       achieved=(nbytes / (ms * 1e-3) / 1e9) if ms else None, peak=PEAK_HBM_GBS, unit="GB/s",
                                       frac=(nbytes / (ms * 1e-3) / 1e9 / PEAK_HBM_GBS) if ms else None, launches=n, avg_ms=ms, bytes_per_launch=nbytes,
                                       traffic=table.get("train_cell_bwd"), traffic_unit="bytes/launch", traffic_source=table.get("_source"),
                                       mfma_util_pmc=(table.get("_mfma_util") or {}).get("train_cell_bwd"),
                                       share_of_step=share, share_unit="ms of one profiled step (HIP events, side stream off)")
            else:
                chans = key.split(" ")[2].split("->") if key.startswith("conv_bf16") else ["64", "64"]
                nbytes = (int(chans[0]) + int(chans[1])) * H * W * 4.0            # x in, y out: fp32 tensors in HBM, rounded to bf16 by the tile loader
                res["roofline"] = dict(bound="hbm", kernel=f"{key} -- the kernel with the largest share of a training step",
                                       achieved=(nbytes / (ms * 1e-3) / 1e9) if ms else None, peak=PEAK_HBM_GBS, unit="GB/s",
                                       frac=(nbytes / (ms * 1e-3) / 1e9 / PEAK_HBM_GBS) if ms else None, launches=n, avg_ms=ms, bytes_per_launch=nbytes, traffic=None,
                                       share_of_step=share, share_unit="ms of one profiled step (HIP events)")
        try:
            import oracle
            from mridc_amd import autograd as ag2
            ncores, box_cores = _oracle_threads()
            cfg1 = dict(cfg, num_cascades=1)
            torch.manual_seed(0)
            model1 = CIRIM(cfg1)                                             # = cascade 0 of the benchmarked model (same seed, same init order)
            state1 = {k: v.detach().clone() for k, v in model1.state_dict().items()}
            host = {k: batch[k].cpu() for k in batch}
            T_ = oracle.models.cirim_time_steps(cfg["time_steps"])
            with torch.no_grad():
                oracle.rim.log_likelihood_gradient(torch.zeros(1, H, W, 2), host["y"], host["sensitivity_maps"], host["mask"], 1.0, cfg["fft_centered"],
                                                   cfg["fft_normalization"], cfg["spatial_dims"], cfg["coil_dim"])      # thread-pool warm-up
            prm = {k: v.clone().requires_grad_(True) for k, v in state1.items()}
            t0 = time.perf_counter()
            pred = oracle.models.cirim_forward(prm, cfg1, host["y"], host["sensitivity_maps"], host["mask"], None, host["target"])
            ref_loss = oracle.models.cirim_process_loss(host["target"], pred, torch.nn.L1Loss(), T_, 1)
            ref_loss.backward()
            dt = time.perf_counter() - t0
            res["cpu_baseline"] = dict(value=1.0 / (dt * cfg["num_cascades"]), unit="slices/s", cores=ncores, kind="port", box_cores=box_cores,
                                       cpu_model=cpu_model_name(),
                                       sample=f"forward + l1 loss + backward (torch autograd) of ONE of the {cfg['num_cascades']} cascades on the oracle, fp32, "
                                              f"{ncores} threads, {dt:.1f} s, extrapolated x{cfg['num_cascades']} (cascades are detached from each other: the cost is linear)")
            model1 = model1.to(dev).train()
            ag2.set_precision(args.dtype)
            for q_ in model1.parameters():
                q_.grad = None
            l1 = training.cirim_forward_backward(model1, batch, args.dtype)
            names = [n_ for n_, _ in model1.named_parameters() if not n_.endswith("dc_weight")]
            g_all = {n_: dict(model1.named_parameters())[n_].grad.detach().cpu().reshape(-1).double() for n_ in names}
            got = torch.cat([g_all[n_] for n_ in names])
            # the checkers (oracle/amp.py): fp32 autograd above; for bf16 also the reference's AMP arithmetic as torch.autocast, and the kernels' own
            # arithmetic (bf16 operands and bf16 results restated on the CPU): the tight one -- it differs from the kernels by the order of fp32 sums only
            checks_ = {"fp32": (ref_loss.detach(), {k_: v_.grad for k_, v_ in prm.items() if v_.grad is not None})}
            if args.dtype == "bf16":
                checks_["autocast_bf16"] = oracle.amp.cirim_loss_and_gradients(state1, cfg1, host, "autocast_bf16")
                emul = dict(round_results=True) if training.BF16_STORAGE else dict(fp32_forward=((64, 2),))
                checks_["kernel_arithmetic"] = oracle.amp.cirim_loss_and_gradients(state1, cfg1, host, "bf16_operands", **emul)
            errs = {}
            for m_, (rl_, gr_) in checks_.items():
                want = torch.cat([gr_[n_].reshape(-1).double() for n_ in names])
                errs[m_] = dict(rel_l2=float((got - want).norm() / want.norm()), loss_rel=abs(float(l1) - float(rl_)) / abs(float(rl_)))
            flat_ = {m_: torch.cat([gr_[n_].reshape(-1).double() for n_ in names]) for m_, (_, gr_) in checks_.items()}
            ms_ = list(flat_)
            oracle_vs_oracle = {f"{a_}_vs_{b_}": float((flat_[a_] - flat_[b_]).norm() / flat_[b_].norm()) for i_, a_ in enumerate(ms_) for b_ in ms_[i_ + 1:]}
            tight = "kernel_arithmetic" if args.dtype == "bf16" else "fp32"
            tol = TRAIN_TOL[args.dtype]
            res["parity_vs_oracle"] = dict(rel_l2=errs[tight]["rel_l2"], loss_rel=errs[tight]["loss_rel"], against=tight, all=errs, tolerance=tol, oracle_vs_oracle=oracle_vs_oracle,
                                           within_tolerance=all(errs[m_]["rel_l2"] <= tol[m_] for m_ in errs),
                                           margin={m_: (tol[m_] / errs[m_]["rel_l2"]) if errs[m_]["rel_l2"] > 0 else None for m_ in errs},   # tolerance / measured: how much room each bound leaves
                                           per_tensor_rel_l2={m_: {n_: float((g_all[n_] - gr_[n_].reshape(-1).double()).norm() / gr_[n_].reshape(-1).double().norm())
                                                                   for n_ in names} for m_, (_, gr_) in checks_.items()},
                                           at=f"whole gradient vector ({got.numel()} parameters) and loss of one cascade (8 time-steps) at {C} x {H} x {W}, {args.dtype}: "
                                              "HIP tape against torch autograd of the oracle in each arithmetic of oracle/amp.py (fp32; autocast_bf16 = the reference's "
                                              "`precision: 16` semantics on the CPU; kernel_arithmetic = bf16 operands and bf16 convolution results, fp32 sums: what the "
                                              "kernels compute); the same tolerances are asserted by tests/test_gpu_headline.py::test_one_cascade_training_at_headline_size "
                                              "on two sets of weights")
        except Exception as ex:  # noqa: BLE001
            res["cpu_baseline"] = dict(value=None, unit="slices/s", cores=os.cpu_count(), kind="port", sample=f"failed: {type(ex).__name__}: {ex}")
    return res


# Whole-gradient rel-L2 of the training tape against each oracle arithmetic (oracle/amp.py), met by the bench's seed-0 weights AND the tests' weights:
#   kernel_arithmetic -- the kernels' own rounding points restated on the CPU.  Results that are ROUNDED to bf16 make the gradient discontinuous in the
#                        order of the fp32 sums (a flipped rounding moves a ReLU mask): two CPU restatements of this very arithmetic that differ only in
#                        accumulating in fp32 or fp64 are 5e-3 apart on the bench's weights, in exactly the parameters where the kernels deviate
#                        (profiles/r04_training_parity_notes.md) on the BOOSTED weights; on the bench's own (seed 0) the tape sits 3.5e-4 from it, bounded
#                        here at 3e-3 (round 5: near the measurement, with the margin reported); what IS exact up to rounding flips is every kernel
#                        on its own (tests/test_gpu_train_bf16.py) and the fp32 tape (1e-5 here);
#   autocast_bf16     -- torch.autocast on the host CPU (the reference's semantics; also accumulates a weight's gradient over the time-steps in bf16);
#   fp32              -- what bf16 costs (the autocast oracle itself sits 1e-2 .. 8e-2 from the fp32 one).
TRAIN_TOL = dict(f32=dict(fp32=2e-3), bf16=dict(kernel_arithmetic=3e-3, autocast_bf16=6e-3, fp32=1e-1))
_RESULT = []


def summary_of(res):
    """<= 1 KB digest of every configuration on the line, appended as its LAST key so that a reader who keeps only the tail of the line (the
    driver's record does) still has each config's value, its dominant kernel's roofline fraction, counter traffic over algorithmic bytes, parity
    and CPU baseline."""
    def r3(v):
        return None if v is None else float(f"{v:.4g}")

    def one(r):
        if not isinstance(r, dict):
            return None
        rf = r.get("roofline") or {}
        tr, ab = rf.get("traffic"), rf.get("algorithmic_bytes") or rf.get("bytes_per_call")
        par = r.get("parity_vs_oracle") or r.get("parity") or {}
        rel = par.get("rel_l2") if isinstance(par, dict) else None
        if rel is None and isinstance(par, dict):
            rel = par.get("grad_rel_l2_vs_kernel_arithmetic") or par.get("rel_l2_vs_kernel_arithmetic")
        cb = r.get("cpu_baseline") or {}
        smin = cb.get("sec_per_slice_min")      # the fastest slice of the CPU sample beside the mean: the box-to-box spread is 1.7x
        return dict(v=r3(r.get("value")), ms=r3(r.get("ms_per_step")), frac=r3(rf.get("frac")), bound=rf.get("bound"),
                    traf=r3(tr / ab) if (tr and ab) else None, rel=r3(rel), cpu=r3(cb.get("value")), cpu_max=r3(1.0 / smin) if smin else None,
                    err=r.get("error"))
    out = {"headline": one(res)}
    out["headline"]["fft_frac"] = r3((res.get("roofline_fft") or {}).get("frac"))
    out["headline"]["fft_exec_frac"] = r3((res.get("roofline_fft") or {}).get("executed_frac"))
    out["headline"]["mfma_busy_reg"] = r3((res.get("roofline") or {}).get("mfma_util_pmc_regulariser"))
    if isinstance(res.get("exact_fp32_route"), dict):
        out["bf16x3"] = dict(v=r3(res["exact_fp32_route"].get("value")))
    if isinstance(res.get("streamed_inputs"), dict):
        out["streamed"] = dict(v=r3(res["streamed_inputs"].get("value")))
    short = {"e2evn_6cascade_15coil_640x372": "e2evn", "qcirim_4echo_32coil_256x256": "qcirim", "cirim_training_bf16_15coil_640x372": "train_bf16",
             "e2evn_training_15coil_640x372": "train_e2evn", "cirim_2d_mask_15coil_640x372": "mask2d", "cirim_precision16_15coil_640x372": "prec16", "e2evn_precision16_15coil_640x372": "e2evn16", "qcirim_precision16_4echo_32coil_256x256": "qcirim16",
             "cirim_8cascade_x5_time_steps_rimblock_direct": "rim5"}
    for k, r in (res.get("other_configs") or {}).items():
        out[short.get(k, k)] = {a: b for a, b in (one(r) or {}).items() if b is not None}
    out["headline"] = {a: b for a, b in out["headline"].items() if b is not None}
    return out


def emit(res):
    """Keep the result line until the very end of the run: it is printed after the process group is gone and the C runtime's buffered
    output (RCCL prints its library path through stdio) has been flushed, so the JSON line is the last line on stdout."""
    _RESULT.append(res)


LINE_LIMIT = 7500        # characters of the stdout line (the driver parsed 19.8 KB in round 4 and not 24.9 KB in round 5: stay far below, under an 8 KB tail)
DETAIL_FILE = "bench_detail.json"

_ROOFLINE_KEYS = ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "launches", "avg_ms", "algorithmic_bytes", "bytes_per_call",
                  "executed_frac", "hbm_frac", "mfma_util_pmc", "mfma_util_pmc_regulariser", "flops_per_launch", "mfma_flops_per_launch")
_CPU_KEYS = ("value", "unit", "cores", "kind", "sample", "sec_per_slice_min", "sec_per_slice_mean", "value_max")
_PARITY_KEYS = ("rel_l2", "ssim", "nmse", "within_tolerance", "grad_rel_l2_vs_kernel_arithmetic", "rel_l2_vs_kernel_arithmetic", "loss_rel_err")


def _num(v):
    return float(f"{v:.6g}") if isinstance(v, float) else v


def _pick(d, keys, cap):
    if not isinstance(d, dict):
        return d
    out = {}
    for k in keys:
        if k in d and d[k] is not None:
            v = d[k]
            if isinstance(v, str):
                v = v if len(v) <= cap else v[:cap - 3] + "..."
            elif isinstance(v, (dict, list)):
                continue
            out[k] = _num(v)
    return out


def compact_line(res, limit=LINE_LIMIT):
    """What goes on stdout: the contract's fixed keys, `config`, `roofline` (numbers + a <= 200-character kernel name), `cpu_baseline` (no
    per-cascade lists), the parity numbers, one short record per other configuration and `summary` as the LAST key -- <= `limit` characters, asserted
    by tests/test_host_logic.py.  Everything else (notes, per-tensor tables, event calibration) goes to DETAIL_FILE and stderr."""
    fixed = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data")
    out = {k: _num(res.get(k)) for k in fixed if k in res}
    cfg = res.get("config") or {}
    out["config"] = {k: (v if not isinstance(v, str) or len(v) <= 260 else v[:257] + "...") for k, v in cfg.items()
                     if isinstance(v, (str, int, float, bool)) and k != "arith"}
    for k in ("world_size_seen", "launch", "concurrent_replays_bit_identical_to_serial"):
        if k in res:
            out[k] = res[k]
    if isinstance(res.get("per_rank_ms_per_step"), list) and len(res["per_rank_ms_per_step"]) <= 8:
        out["per_rank_ms_per_step"] = [_num(float(v)) for v in res["per_rank_ms_per_step"]]
    if isinstance(res.get("roofline"), dict):
        out["roofline"] = _pick(res["roofline"], _ROOFLINE_KEYS, 200)
    if isinstance(res.get("roofline_fft"), dict):
        out["roofline_fft"] = _pick(res["roofline_fft"], _ROOFLINE_KEYS, 120)
    if isinstance(res.get("breakdown_ms"), dict):
        out["breakdown_ms"] = {k: _num(v) for k, v in res["breakdown_ms"].items() if isinstance(v, (int, float))}
    if isinstance(res.get("cpu_baseline"), dict):
        out["cpu_baseline"] = _pick(res["cpu_baseline"], _CPU_KEYS, 220)
    if isinstance(res.get("parity_vs_oracle"), dict):
        out["parity_vs_oracle"] = _pick(res["parity_vs_oracle"], _PARITY_KEYS, 80)
    for k in ("exact_fp32_route", "streamed_inputs"):
        if isinstance(res.get(k), dict):
            out[k] = _pick(res[k], ("value", "unit", "ms_per_step"), 40)
    others = {}
    for name, r in (res.get("other_configs") or {}).items():
        if not isinstance(r, dict):
            continue
        o = _pick(r, ("value", "unit", "ms_per_step", "dtype", "steps", "warmup", "error"), 160)
        if isinstance(r.get("roofline"), dict):
            o["roofline"] = _pick(r["roofline"], ("bound", "achieved", "peak", "unit", "frac", "traffic", "avg_ms"), 60)      # (the kernel names: DETAIL_FILE)
        if isinstance(r.get("cpu_baseline"), dict):
            o["cpu_baseline"] = _pick(r["cpu_baseline"], ("value", "unit", "cores", "kind"), 40)
        par = r.get("parity_vs_oracle") or r.get("parity")
        if isinstance(par, dict):
            o["parity"] = _pick(par, _PARITY_KEYS, 40)
        others[name] = o
    if others:
        out["other_configs"] = others
    out["detail"] = DETAIL_FILE
    if "summary" in res:
        out["summary"] = res["summary"]
    # never let the line outgrow the limit: shed the optional sections, least important first (`summary` keeps every configuration's value)
    for drop in ("breakdown_ms", "per_rank_ms_per_step", "exact_fp32_route", "streamed_inputs", "roofline_fft", "other_configs"):
        if len(json.dumps(out)) <= limit:
            break
        out.pop(drop, None)
    return out


def flush_result():
    import ctypes
    try:
        ctypes.CDLL(None).fflush(None)
    except Exception:  # noqa: BLE001
        pass
    for res in _RESULT:
        full = json.dumps(res)
        try:
            with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), DETAIL_FILE), "w") as f:
                f.write(full + "\n")
            out_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpurun_out")
            if os.path.isdir(out_dir):
                with open(os.path.join(out_dir, DETAIL_FILE), "w") as f:
                    f.write(full + "\n")
        except OSError:
            pass
        if os.environ.get("MRX_BENCH_DETAIL_STDERR") == "1":      # (opt-in: a driver that merges stderr into its tail should see the short line only)
            print("[bench detail] " + full, file=sys.stderr, flush=True)
        print(json.dumps(compact_line(res)), flush=True)
    _RESULT.clear()


def dist_barrier(sync=True):
    """Barrier over the ranks (when a process group exists) + device synchronize."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        dist.barrier()
    if sync:
        torch.cuda.synchronize()


def rank_times(elapsed, dev):
    """(max over ranks, [every rank's elapsed seconds]) -- one all-gather of a double per rank."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        every = [torch.zeros_like(t) for _ in range(dist.get_world_size())]
        dist.all_gather(every, t)
        per_rank = [float(v.item()) for v in every]
        return max(per_rank), per_rank
    return elapsed, [elapsed]


def max_over_ranks(elapsed, dev):
    return rank_times(elapsed, dev)[0]


def world_seen():
    import torch.distributed as dist
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def measured_traffic(B, C, H, W, F):
    """HBM bytes per launch of the hot kernels from the newest committed PMC passes (profiles/r*_traffic.json: FETCH_SIZE and
    WRITE_SIZE, one counter per rocprofv3 pass, gfx950 correction applied; written by tools/traffic_json.py).  Counter collection
    cannot run inside the timed bench (~0.3 s per dispatch), so the numbers are reported only when this run has the shape AND the
    library version (mrx_version: bumped with every kernel change) they were measured with -- otherwise `traffic` is null."""
    import glob
    from mridc_amd import _lib
    paths = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "r*_traffic*.json")))      # (rNN_traffic.json: one slice per launch; rNN_traffic_b8.json: the default line's 8)
    for path in reversed(paths):
        try:
            with open(path) as f:
                t = json.load(f)
        except (OSError, ValueError):
            continue
        if t.get("shape") != dict(batch=B, coils=C, height=H, width=W, features=F) or t.get("lib_version") != int(_lib.lib().mrx_version()):
            continue
        out = {k: v["hbm_bytes_per_launch"] for k, v in t["kernels"].items()}
        out["_kernels"] = {k: v["kernel"] for k, v in t["kernels"].items()}
        out["_mfma_util"] = {k: v.get("mfma_util") for k, v in t["kernels"].items()}     # SQ_VALU_MFMA_BUSY_CYCLES / (4 x SQ_BUSY_CU_CYCLES)
        out["_mfma_util"]["regulariser"] = t.get("regulariser_mfma_util")
        out["_mfma_util_source"] = t.get("_mfma_util")
        out["_source"] = f"profiles/{os.path.basename(path)} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes, 2 x FETCH + WRITE)"
        return out
    return {}


def exact_route_line(args):
    """The headline in a CHILD process with the layer kernels on three-term bf16 operands (six exact term products per fp32 multiply,
    error O(2^-24): the route the two-term fp16 default is judged against).  A child because the route is chosen once per process."""
    import subprocess
    env = dict(os.environ, MRIDC_AMD_ARITH="bf16x3")
    cmd = [sys.executable, os.path.abspath(__file__), "--full", "--no-cpu-baseline", "--no-other-configs", "--no-stream-inputs", "--steps", "6", "--warmup", "2",
           "--coils", str(args.coils), "--height", str(args.height), "--width", str(args.width), "--mask", args.mask]
    try:
        out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
        r = json.loads(line)
        return dict(value=r["value"], unit=r["unit"], ms_per_step=r["ms_per_step"], breakdown_ms=r.get("breakdown_ms"),
                    arith="three bf16 terms per fp32 operand, six term products per multiply on v_mfma_f32_32x32x16_bf16, fp32 accumulation "
                          "(MRIDC_AMD_ARITH=bf16x3)", steps=r["steps"])
    except Exception as ex:  # noqa: BLE001
        return dict(value=None, error=f"{type(ex).__name__}: {ex}")


def training_line(args, model="cirim"):
    """BASELINE config 4 (CIRIM training, bf16) in a CHILD process: run inside this process after the inference benches the same step measured
    15-16 slices/s against 23 in a fresh process (allocator and stream state left by the graphs of the three inference runs), and a number that depends
    on what ran before it is not a measurement.  The child's whole record (roofline on the cell-backward kernel, parity against the three oracle
    arithmetics, CPU baseline) rides along."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--full", "--train", "--dtype", "bf16", "--steps", "4", "--warmup", "1", "--no-other-configs", "--no-stream-inputs",
           "--coils", str(args.coils), "--height", str(args.height), "--width", str(args.width)] + (["--no-cpu-baseline"] if args.no_cpu_baseline else [])
    if model == "e2evn":        # E2EVN under the same trainer: forward + loss + backward as one hipGraph replay
        cmd = [sys.executable, os.path.abspath(__file__), "--full", "--train", "--model", "e2evn", "--steps", "6", "--warmup", "2", "--no-other-configs", "--no-stream-inputs",
               "--no-cpu-baseline", "--coils", str(args.coils), "--height", str(args.height), "--width", str(args.width)]
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        r = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
        for drop in ("n_gpus", "higher_is_better", "scaling", "vs_baseline", "world_size_seen", "per_rank_ms_per_step", "data"):
            r.pop(drop, None)
        r["process"] = "child (fresh process)"
        return r
    except Exception as ex:  # noqa: BLE001
        return dict(value=None, error=f"{type(ex).__name__}: {ex}")


def rim5_line(args):
    """SURVEY 0.4's second figure: the eight cascades with FIVE time-steps each -- what RIMBlock(time_steps=5) runs when it is called directly
    (models/rim/rim_block.py:68,217); CIRIM rounds its config's 5 up to 8 (models/cirim.py:50-51: the headline).  A child process."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--full", "--no-cpu-baseline", "--no-other-configs", "--no-stream-inputs", "--steps", "8", "--warmup", "2",
           "--coils", str(args.coils), "--height", str(args.height), "--width", str(args.width), "--rim-steps", "5"]
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        r = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
        return dict(metric=r["metric"] + ", 5 time-steps per RIMBlock call", value=r["value"], unit=r["unit"], ms_per_step=r["ms_per_step"], steps=r["steps"],
                    warmup=r["warmup"], config=r.get("config"), breakdown_ms=r.get("breakdown_ms"))
    except Exception as ex:  # noqa: BLE001
        return dict(value=None, error=f"{type(ex).__name__}: {ex}")


def mask2d_line(args):
    """The headline with a row-dependent (2-D) sampling mask -- the family of the reference's default CIRIM configuration (Poisson-2D,
    base_cirim_run.yaml:84-90): the data-consistency gradient is then the three-pass kernel chain.  A child process (a fresh model, no state shared
    with the 1-D run); its own roofline_fft record rides along."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--full", "--no-cpu-baseline", "--no-other-configs", "--no-stream-inputs", "--steps", "8", "--warmup", "2",
           "--coils", str(args.coils), "--height", str(args.height), "--width", str(args.width), "--mask", "2d"]
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        r = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
        return dict(metric=r["metric"] + ", 2-D mask", value=r["value"], unit=r["unit"], ms_per_step=r["ms_per_step"], steps=r["steps"], warmup=r["warmup"],
                    config=r.get("config"), breakdown_ms=r.get("breakdown_ms"), roofline=r.get("roofline_fft"),
                    concurrent_replays_bit_identical_to_serial=r.get("concurrent_replays_bit_identical_to_serial"))
    except Exception as ex:  # noqa: BLE001
        return dict(value=None, error=f"{type(ex).__name__}: {ex}")


def streamed_inputs_run(args, step, hosts, datas, dev, slices_per_step, variant="full"):
    """The headline with a new slice per replay: (y, S, mask, target) of the NEXT slice travel from pinned host memory to a staging
    buffer on a copy stream while the current one reconstructs; the compute stream then copies staging -> the graph's static inputs
    (device to device, inside the stream order) and replays.  Reports slices/s beside the resident-input figure."""
    NS = len(datas)
    keys = ("y", "sensitivity_maps", "mask", "target")
    pinned = [{k: h_[k].contiguous().pin_memory() for k in keys} for h_ in hosts]
    staging = [[{k: torch.empty_like(d[k]) for k in keys} for _ in range(2)] for d in datas]      # two staging sets per compute stream
    streams = bench_streams(NS)
    copy_stream = _COPY_STREAM[0] if _COPY_STREAM else _COPY_STREAM.append(torch.cuda.Stream(priority=-1)) or _COPY_STREAM[0]
    graphs = []
    for d, st in zip(datas, streams):
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            step(d)
        torch.cuda.current_stream().wait_stream(st)
        g_ = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_, stream=st, capture_error_mode="thread_local"):
            step(d)
        graphs.append(g_)
    torch.cuda.synchronize()
    landed = [[torch.cuda.Event() for _ in range(2)] for _ in range(NS)]
    freed = [[torch.cuda.Event() for _ in range(2)] for _ in range(NS)]

    def upload(i, slot, src):
        if variant == "no_h2d":
            return
        with torch.cuda.stream(copy_stream):
            copy_stream.wait_event(freed[i][slot])
            for k in keys:
                staging[i][slot][k].copy_(src[k], non_blocking=True)
            landed[i][slot].record(copy_stream)

    for i in range(NS):
        for slot in range(2):
            freed[i][slot].record(streams[i])
        upload(i, 0, pinned[i])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for n in range(args.steps):
        slot = n & 1
        for i, st in enumerate(streams):
            upload(i, slot ^ 1, pinned[(i + n + 1) % NS])              # the slice after this one
            with torch.cuda.stream(st):
                if variant not in ("no_h2d", "no_wait"):
                    st.wait_event(landed[i][slot])
                if variant != "no_d2d":
                    for k in keys:
                        datas[i][k].copy_(staging[i][slot][k], non_blocking=True)
                freed[i][slot].record(st)
                graphs[i].replay()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    nbytes = sum(pinned[0][k].numel() * pinned[0][k].element_size() for k in keys) / max(1, slices_per_step // NS)    # a stream's batch holds slices_per_step / NS slices
    return dict(value=slices_per_step * args.steps / dt, unit="slices/s", ms_per_step=1e3 * dt / args.steps,
                host_to_device_bytes_per_slice=nbytes, host_to_device_GBps=nbytes * slices_per_step * args.steps / dt / 1e9,
                note="every replay reconstructs a slice uploaded during the previous one (pinned host memory -> staging on a copy stream -> the "
                     "graph's static inputs by a device copy in stream order); per-slice operands (lane-ordered maps, IFFT_H(y)) are prepared "
                     "inside the graph")


NUMA_BINDING = None      # {"node", "cpus"} once main() has bound the rank to its GPU's NUMA node
NUMA_BINDING_ALL = None  # the same for every rank (gathered once the process group exists)


def precision16_record(args, cfg, model, state_dict, timer, host, out, elapsed, per_rank, world, NS, B, graphed, conc_ok):
    """The result line of `--precision 16` (the reference's inference configuration, base_cirim_run.yaml:132): both RIM layers are HBM-bound there, so the
    roofline record prices the dominant launch (mrx_amp16_layer2) on its ALGORITHMIC bytes -- x, h_prev in and h_new out as fp16 [B,8,H,W,8], six fp32 tap
    planes out -- against 8 TB/s; `cpu_baseline` and `parity_vs_oracle` are the oracle under torch.autocast(float16)."""
    import oracle
    C, H, W = args.coils, args.height, args.width
    T_, npix, F = model.time_steps, H * W, 64
    ms_per_step = 1e3 * elapsed / args.steps
    value = world * NS * B * args.steps / elapsed
    ms1, n1 = timer.mean_ms("amp_layer1")
    ms2, n2 = timer.mean_ms("amp_layer2")
    msl, nl = timer.mean_ms("llg372")
    msg, ng = timer.mean_ms("llg372g")
    if not msl:
        msl, nl = timer.mean_ms("llg")
    bytes2 = (3.0 * F * 2 + 6 * 4) * npix * B
    bytes1 = (2.0 * F * 2 + 5 * 8) * npix * B            # h_prev in, h out (fp16); eta and four partial planes (complex fp32)
    flops2 = 2.0 * (F * F * 9 + F * F + F * 2 * 9) * npix * B
    traffic = measured_traffic(B, C, H, W, F)
    roofline = dict(bound="hbm", kernel="k_amp_layer2 via mrx_amp16_layer2 (3x3 dilation-2 64->64 + IndRNN 1x1 + the final 3x3's channel contraction; ONE fp16 term "
                                        "per operand on v_mfma_f32_32x32x16_f16, fp32 accumulation, fp16 channel-blocked states)",
                    achieved=(bytes2 / (ms2 * 1e-3) / 1e9) if ms2 else None, peak=PEAK_HBM_GBS, unit="GB/s",
                    frac=(bytes2 / (ms2 * 1e-3) / 1e9 / PEAK_HBM_GBS) if ms2 else None, traffic=traffic.get("amp_layer2"), traffic_unit="bytes/launch",
                    algorithmic_bytes=bytes2, launches=n2, avg_ms=ms2, flops_per_launch=flops2,
                    mfma_frac=(flops2 / (ms2 * 1e-3) / 1e12 / PEAK_BF16_MFMA_TFLOPS) if ms2 else None,
                    layer1=dict(kernel="k_amp_layer1 via mrx_amp16_layer1", avg_ms=ms1, launches=n1, algorithmic_bytes=bytes1,
                                frac=(bytes1 / (ms1 * 1e-3) / 1e9 / PEAK_HBM_GBS) if ms1 else None, traffic=traffic.get("amp_layer1")))
    res = dict(metric=f"slices/sec (inference, precision 16), CIRIM {cfg['num_cascades']}-cascade {C}-coil {H}x{W}", value=value, unit="slices/s", n_gpus=world,
               steps=args.steps, warmup=args.warmup, ms_per_step=ms_per_step, higher_is_better=True, scaling="weak", vs_baseline=None, dtype="f16", data="synthetic",
               config=dict(workload=f"CIRIM {cfg['num_cascades']} cascades x {T_} time-steps, IndRNN {F} filters, {C} coils, {H}x{W}, {NS * B} slice(s) per GPU and step "
                                    f"({NS} concurrent HIP stream(s) x batch {B}, one hipGraph each), random-init weights (seed 0), trainer.precision = 16 "
                                    "(base_cirim_run.yaml:132): fp16 operands + fp16 hidden states in the RIM layers, fp32 accumulation, FFT / DC / eta in fp32",
                           global_batch=world * NS * B, streams_per_gpu=NS, coils=C, height=H, width=W, parallelism=f"slice-sharded x{world}",
                           mask="1-D random columns R=4" if args.mask == "1d" else "2-D random points R~10"),
               world_size_seen=world_seen(), per_rank_ms_per_step=[1e3 * t / args.steps for t in per_rank], launch="hipGraph replay" if graphed else "eager",
               roofline=roofline, breakdown_ms=dict(llg=msl, llg_gather_form=msg, conv_layer1=ms1, conv_layer2=ms2, rim_steps_per_slice=cfg["num_cascades"] * T_),
               concurrent_replays_bit_identical_to_serial=conc_ok)
    if not args.full:                           # a plain run recorded no per-kernel events: no roofline / breakdown records on its line
        for k_ in ("roofline", "breakdown_ms", "concurrent_replays_bit_identical_to_serial"):
            res.pop(k_)
    if args.full and world == 1 and not args.no_cpu_baseline:
        n_cpu = args.cpu_cascades if 0 < args.cpu_cascades <= cfg["num_cascades"] else cfg["num_cascades"]
        try:
            host1 = {k: v[:1] if k != "mask" else v for k, v in host.items()}
            cb, ref = cpu_baseline(cfg, state_dict, host1, n_cpu, args.cpu_slices, ctx=oracle.amp.autocast_fp16, ctx_name=" under torch.autocast(float16)")
            res["cpu_baseline"] = cb
            res["parity_vs_oracle"] = parity_vs_oracle(out[n_cpu - 1][-1][0:1], ref[n_cpu - 1][-1][0:1], host1["target"],
                                                       at=f"cascade {n_cpu} of {cfg['num_cascades']}, last time-step, against the oracle under torch.autocast(float16)")
            res["parity_vs_oracle"]["tolerance"] = dict(rel_l2=3e-2, ssim=0.99, source="SURVEY appendix C, fast mode")
            with torch.no_grad():
                ref32 = oracle.models.cirim_forward(state_dict, dict(cfg, num_cascades=n_cpu), host1["y"], host1["sensitivity_maps"], host1["mask"], None,
                                                    host1["target"])
            res["parity_vs_fp32_oracle"] = parity_vs_oracle(out[n_cpu - 1][-1][0:1], ref32[n_cpu - 1][-1][0:1], host1["target"], at="the same, against the fp32 oracle")
        except Exception as ex:  # noqa: BLE001
            res["cpu_baseline"] = dict(value=None, unit="slices/s", cores=os.cpu_count(), kind="port", sample=f"failed: {type(ex).__name__}: {ex}")
    res["summary"] = summary_of(res)
    return res


def precision16_line(args):
    """BASELINE's headline model in the reference's own inference precision (`trainer.precision: 16`): a child process of the default run."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--full", "--no-other-configs", "--no-stream-inputs", "--steps", "10", "--warmup", "3", "--precision", "16",
           "--coils", str(args.coils), "--height", str(args.height), "--width", str(args.width), "--cpu-slices", "1", "--cpu-cascades", "1"]     # (torch's CPU fp16 convolutions take ~7 s per RIM step on the GPU box's EPYC: one cascade of one slice, extrapolated)
    cmd += ["--no-cpu-baseline"] if args.no_cpu_baseline else []
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        r = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
        return {k: r.get(k) for k in ("metric", "value", "unit", "ms_per_step", "steps", "warmup", "dtype", "config", "roofline", "breakdown_ms", "cpu_baseline",
                                      "parity_vs_oracle", "parity_vs_fp32_oracle", "concurrent_replays_bit_identical_to_serial") if r.get(k) is not None}
    except Exception as ex:  # noqa: BLE001
        return dict(value=None, error=f"{type(ex).__name__}: {ex}")


def main():
    args = parse()
    plan = rank_launch_plan(args.gpus, sys.argv[1:], os.environ)
    if plan is not None:                                  # bare `--gpus N`: this parent only spawns and waits (no GPU call before this)
        sys.exit(spawn_ranks(plan))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and rank == 0:
        print(f"[bench] --gpus {args.gpus} but the launcher started {world} rank(s): reporting n_gpus = {world}", file=sys.stderr)
    if args.dist_selftest:
        dist_selftest(args)
        return
    # the rank on the CPUs (and, by first touch, the memory) of its GPU's NUMA node -- before the first GPU call (MRX_BENCH_NUMA=0 leaves the affinity alone)
    from mridc_amd.sharding import bind_rank_to_gpu_numa_node
    global NUMA_BINDING
    NUMA_BINDING = bind_rank_to_gpu_numa_node(local_rank) if os.environ.get("MRX_BENCH_NUMA", "1") != "0" else None
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the product path has no CPU fallback)")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # MRX_BENCH_FORCE_DIST=1: run the RCCL init / barrier / max-reduce path with a single rank too (a 1-GPU box can then check
    # that the process group and the hipGraph capture get along)
    use_dist = world > 1 or os.environ.get("MRX_BENCH_FORCE_DIST") == "1"
    if use_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        global NUMA_BINDING_ALL
        try:                                                    # every rank's binding on the line, not only rank 0's (a wrong guess pins a rank to the far socket)
            got = [None] * world
            dist.all_gather_object(got, NUMA_BINDING)
            NUMA_BINDING_ALL = got
        except Exception:  # noqa: BLE001
            NUMA_BINDING_ALL = None

    from mridc_amd import ops, synthetic
    from mridc_amd.collections.reconstruction.models.cirim import CIRIM

    if args.train:
        r_ = bench_train(args, world, rank, dev, checks=args.full and world == 1 and not args.no_cpu_baseline)
        if rank == 0:
            emit(r_)
        if use_dist:
            dist.destroy_process_group()
        flush_result()
        return
    if args.model != "cirim":
        r_ = (bench_qcirim if args.model == "qcirim" else bench_e2evn)(args, world, rank, dev, checks=args.full and world == 1 and not args.no_cpu_baseline)
        if rank == 0:
            emit(r_)
        if use_dist:
            dist.destroy_process_group()
        flush_result()
        return
    cfg = dict(synthetic.CIRIM_BASELINE_CFG)
    cfg["recurrent_layer"] = args.rnn
    if args.cascades:
        cfg["num_cascades"] = args.cascades
    torch.manual_seed(0)                                # reference-identical initialisation (tests/test_host_logic.py)
    model = CIRIM(dict(cfg, precision=16) if args.precision == 16 else cfg).eval()
    if args.rim_steps:                                  # the blocks called as RIMBlock(time_steps = N) directly: no rounding up to a multiple of 8
        model.time_steps = args.rim_steps
        for blk in model.cirim:
            blk.time_steps = args.rim_steps
    state_dict = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(dev)
    B, C, H, W = args.batch, args.coils, args.height, args.width
    NS = max(1, args.streams)
    # each rank reconstructs its own contiguous share of the world*NS*B slices: embarrassingly parallel, no collective
    from mridc_amd.sharding import shard_range
    s0, s1 = shard_range(world * NS * B, rank, world)

    all_slices = make_slices(C, H, W, range(s0, s1))

    def make_host(first):
        slices = all_slices[first - s0:first - s0 + B]
        h_ = {k: torch.cat([s[k] for s in slices], 0) for k in ("y", "sensitivity_maps", "target")}
        h_["mask"] = slices[0]["mask"]
        if args.mask == "2d":                           # k-space re-masked with a 2-D pattern (keeps a fully sampled centre)
            g2 = torch.Generator().manual_seed(7)
            m2 = torch.rand(1, 1, H, W, 1, generator=g2) < 0.08
            m2[:, :, :16, :16] = True
            m2[:, :, -16:, :16] = True
            m2[:, :, :16, -16:] = True
            m2[:, :, -16:, -16:] = True
            h_["mask"] = m2
            h_["y"] = torch.cat([s["kspace"] for s in slices], 0) * m2
        return h_

    assert s0 + NS * B == s1
    hosts = [make_host(s0 + i * B) for i in range(NS)]
    del all_slices
    host = hosts[0]
    datas = [{k: v.to(dev) for k, v in h_.items()} for h_ in hosts]
    data = datas[0]
    from mridc_amd import _lib
    _lib.check(_lib.lib().mrx_fft_prepare(H, W), "mrx_fft_prepare")

    timer = KernelTimer()
    F_hidden = cfg["recurrent_filters"][0]
    timer.wrap(ops, "rim_layer_indrnn", lambda x, *a, **k: "conv_layer2" if x.shape[1] == F_hidden else "conv_layer1")
    timer.wrap(ops, "rim_layer_indrnn_packed", lambda x, *a, **k: "conv_layer2" if x.shape[1] == F_hidden else "conv_layer1")
    timer.wrap(ops, "rim_layer_indrnn_wino", lambda x, *a, **k: "conv_layer2_wino")
    timer.wrap(ops, "rim_layer2_sb", lambda x, *a, **k: "conv_layer2_sb")
    timer.wrap(ops, "rim_layer2_sb_taps", lambda x, *a, **k: "conv_layer2_sbt")     # + the final convolution's channel contraction in its tail
    timer.wrap(ops, "rim_layer2_f16", lambda x, *a, **k: "conv_layer2_f16t" if k.get("want_taps") else "conv_layer2_f16")   # two-term fp16 conv operands
    timer.wrap(ops, "rim_layer2_f16_cb8", lambda x, *a, **k: "conv_layer2_f16t" if k.get("want_taps") else "conv_layer2_f16")   # channel-blocked states
    timer.wrap(ops, "rim_layer2_f16_cb8_q", lambda *a, **k: "conv_layer2_f16t")     # ... with the tap products pre-summed along x (6 planes + tile-edge terms)
    timer.wrap(ops, "amp16_layer1", lambda *a, **k: "amp_layer1")                  # --precision 16: fp16 operands and states (csrc/rim_amp16.hip)
    timer.wrap(ops, "amp16_layer2", lambda *a, **k: "amp_layer2")
    timer.wrap(ops, "rim_final_gather_q", lambda *a, **k: "final_gather")
    timer.wrap(ops, "llg372_gather_q", lambda *a, **k: "llg372g")
    timer.wrap(ops, "rim_layer1_cb8", lambda *a, **k: "conv_layer1")
    timer.wrap(ops, "rim_final_gather", lambda *a, **k: "final_gather")
    timer.wrap(ops, "llg", lambda *a, **k: "llg")
    timer.wrap(ops, "llg_hinv", lambda *a, **k: "llg")
    timer.wrap(ops, "llg_hinv_parts", lambda *a, **k: "llg")     # gradient whose last pass is done by layer 1's tile loader
    timer.wrap(ops, "llg372", lambda *a, **k: "llg372")          # W = 372: wave-private prime-factor transforms, one launch
    timer.wrap(ops, "llg372_gather", lambda *a, **k: "llg372g")  # ... with the previous step's nine-tap gather (eta + final convolution) folded in
    timer.wrap(ops, "rim_layer_indrnn_packed_llg", lambda *a, **k: "conv_layer1")
    timer.wrap(ops, "rim_final", lambda *a, **k: "final")

    def step(d=None):
        d = data if d is None else d
        with torch.no_grad():
            return next(model(d["y"], d["sensitivity_maps"], d["mask"], None, d["target"]))

    barrier = dist_barrier

    out = None
    for _ in range(max(args.warmup, 1)):
        out = step()
    # Launch-bound inner loop (392 dependent kernels per step): capture the step once and replay it as a hipGraph.
    # Per-kernel HIP events cannot be recorded inside a replay, so the kernel breakdown (--full) is measured on eager steps first.
    if args.full:
        timer.enabled = True
        barrier()
        try:
            # the host needs ~10 us per eager launch, several kernels take less: park the GPU behind a spin kernel while the two timed steps
            # are enqueued, so that every event pair brackets GPU execution and not the host's launch latency
            torch.cuda._sleep(int(4e7))
        except Exception:  # noqa: BLE001
            pass
        for _ in range(2):
            step()
        timer.calibrate()
        barrier()
        timer.enabled = False
    # One captured hipGraph per stream (392 dependent kernels per slice are launch-bound when issued eagerly).  Per-kernel HIP
    # events cannot be recorded inside a replay, so the kernel breakdown above was measured on eager steps.
    streams = bench_streams(NS)
    graphs, graphed, outs = [], False, [None] * NS
    if args.graph:
        try:
            for i, (d, st) in enumerate(zip(datas, streams)):
                st.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(st):
                    step(d)
                torch.cuda.current_stream().wait_stream(st)
                g_ = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g_, stream=st, capture_error_mode="thread_local"):
                    outs[i] = step(d)
                graphs.append(g_)
            for g_, st in zip(graphs, streams):
                with torch.cuda.stream(st):
                    g_.replay()
            torch.cuda.synchronize()
            graphed = True
            out = outs[0]
        except Exception as ex:  # noqa: BLE001
            print(f"[bench] hipGraph capture unavailable ({type(ex).__name__}: {ex}); timing eager launches", file=sys.stderr)
            graphs = []
            torch.cuda.synchronize()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        for i, st in enumerate(streams):
            with torch.cuda.stream(st):
                if graphs:
                    graphs[i].replay()
                else:
                    outs[i] = step(datas[i])
                    if i == 0:
                        out = outs[i]
    barrier()
    elapsed, per_rank = rank_times(time.perf_counter() - t0, dev)
    if args.dump_outputs and rank == 0:
        write_outputs(args.dump_outputs, outs)
    headline_conc_ok = concurrent_replays_match_serial(graphs, streams, outs) if args.full else None

    if rank == 0 and args.precision == 16:
        emit(precision16_record(args, cfg, model, state_dict, timer, host, out, elapsed, per_rank, world, NS, B, graphed, headline_conc_ok))
    elif rank == 0:
        T_ = model.time_steps
        npix = H * W
        ms_per_step = 1e3 * elapsed / args.steps
        value = world * NS * B * args.steps / elapsed
        # dominant kernel: fused layer 2 = conv3x3 dil2 (64->64) + 1x1 ih (64->64): 2*(64*64*9 + 64*64) flop / pixel (SURVEY 8d,
        # direct-form count).  The Winograd form issues 2*(64*64*4 + 64*64) of MFMA work for it: `achieved` / `frac` are what the
        # matrix pipe actually executes (a fraction of the fp32-MFMA peak, never above 1); the direct-form rate is kept beside them
        # as `algorithmic_*` (the saving of the algorithm, not pipe utilisation).
        flops2 = 2.0 * (F_hidden * F_hidden * 9 + F_hidden * F_hidden) * npix * B
        ms2, n2 = timer.mean_ms("conv_layer2")
        kname = "k_rim_layer<3,2,8> (conv3x3 d2 64->64 + IndRNN 1x1 fused, fp32 MFMA 32x32x2)"
        executed = flops2
        msw, nw = timer.mean_ms("conv_layer2_wino")
        if msw:
            ms2, n2 = msw, nw
            kname = ("k_rim_layer_wino (conv3x3 d2 64->64 as Winograd F(2x2,3x3) on the parity sub-lattices + IndRNN 1x1 fused, "
                     "fp32 MFMA 16x16x4 / 32x32x2)")
            executed = 2.0 * (F_hidden * F_hidden * 4 + F_hidden * F_hidden) * npix * B
        peak2, l2_bf16 = PEAK_FP32_MFMA_TFLOPS, False
        mss, nss = timer.mean_ms("conv_layer2_sb")
        if mss:                               # the default: direct convolution on the bf16 matrix pipe, fp32 results (three-term operand split)
            ms2, n2, l2_bf16, peak2 = mss, nss, True, PEAK_BF16_MFMA_TFLOPS
            kname = ("k_rim_layer2_sb (conv3x3 d2 64->64 direct form + IndRNN 1x1 fused; every fp32 operand = 3 bf16 terms, 6 term products per "
                     "multiply on v_mfma_f32_32x32x16_bf16, fp32 accumulation: fp32-accurate results; 36 steps of 2 taps x 8 channels (the ninth taps of "
                     "two consecutive channel chunks share a step: no padding) + 4 steps of the 1x1 stage = 480 MFMAs per 32 pixels)")
            executed = (480 * 32 * 32 * 16 * 2 / 32.0) * npix * B
        mst, nst = timer.mean_ms("conv_layer2_sbt")
        l2_taps = bool(mst)
        if mst:                               # the same kernel with the final 64 -> 2 convolution's channel contraction in its tail (+ 24 MFMAs per 32 pixels)
            ms2, n2, l2_bf16, peak2 = mst, nst, True, PEAK_BF16_MFMA_TFLOPS
            kname = ("k_rim_layer2_sb (conv3x3 d2 64->64 direct form + IndRNN 1x1 fused + the channel contraction of the final 3x3 64->2 convolution "
                     "on the new state (18 tap-product planes; mrx_rim_final_gather adds the shifted taps); every fp32 operand = 3 bf16 terms, 6 term "
                     "products per multiply on v_mfma_f32_32x32x16_bf16, fp32 accumulation: fp32-accurate results; 36 steps of 2 taps x 8 channels (the "
                     "ninth taps of two consecutive channel chunks share a step: no padding) + 4 steps of the 1x1 stage + 4 steps of the tap stage "
                     "(18 of 32 rows used) = 504 MFMAs per 32 pixels)")
            executed = (504 * 32 * 32 * 16 * 2 / 32.0) * npix * B
            flops2 += 2.0 * F_hidden * 2 * 9 * npix * B      # the final convolution's multiply-adds now belong to this launch
        msh, nsh = timer.mean_ms("conv_layer2_f16t")
        l2_f16 = bool(msh)
        if msh:                               # the default: the convolution's operands as two fp16 terms, three term products per multiply
            ms2, n2, l2_bf16, peak2, l2_taps = msh, nsh, True, PEAK_BF16_MFMA_TFLOPS, True
            kname = ("k_rim_layer2_sb<.., F16, CB8> (hidden states channel-blocked [B,8,H,W,8]; conv3x3 d2 64->64 direct form + IndRNN 1x1 fused + the channel contraction of the final 3x3 64->2 "
                     "convolution on the new state; convolution operands = 2 fp16 terms scaled by powers of two (x by the bound of its maximum that "
                     "layer 1 keeps, w at pack time), 3 term products per multiply on v_mfma_f32_32x32x16_f16, fp32 accumulation: error against "
                     "float64 2.3e-7 (three-term bf16 form 2.8e-7, fp32 Winograd 2.0e-7); 36 steps x 6 MFMAs + the 1x1 and tap stages with two fp16 terms "
                     "scaled per pixel (4 steps x 6 + 4 steps x 3) = 252 MFMAs per 32 pixels; fp16 and bf16 MFMAs issue at the same rate, priced "
                     "against the same dense peak)")
            executed = (252 * 32 * 32 * 16 * 2 / 32.0) * npix * B
            flops2 += 2.0 * F_hidden * 2 * 9 * npix * B
        traffic = measured_traffic(B, C, H, W, F_hidden)
        tf = (lambda fl: fl / (ms2 * 1e-3) / 1e12) if ms2 else (lambda fl: None)
        ms1, _ = timer.mean_ms("conv_layer1")
        msf, _ = timer.mean_ms("final")
        if l2_taps:
            msf, _ = timer.mean_ms("final_gather")
        msl, nl = timer.mean_ms("llg")
        ms372, n372 = timer.mean_ms("llg372")
        ms372g, n372g = timer.mean_ms("llg372g")
        if ms372:
            msl, nl = ms372, n372
        # per RIM step: the gradient launch (7 of 8 steps of a cascade in the form that also does the previous step's tap gather) and what is left of
        # the stand-alone gather (the last step of every cascade)
        steps_prof = float((n372 or 0) + (n372g or 0)) or None
        llg_per_step = (((ms372 or 0.0) * (n372 or 0) + (ms372g or 0.0) * (n372g or 0)) / steps_prof) if (steps_prof and ms372) else msl
        n_fin = timer.mean_ms("final_gather")[1] if l2_taps else 0
        final_per_step = (msf * n_fin / steps_prof) if (steps_prof and msf and n_fin and n372g) else msf
        # whole regulariser (layer 1 + layer 2 + final conv) as issued on the matrix / vector pipes.  Layer 1 runs on the bf16 matrix pipe
        # (k_rim_layer1_sb: three-term bf16 operand split, 6 term products per multiply, 132 MFMAs of 32x32x16 per 32 pixels) unless
        # MRIDC_AMD_ARITH=fp32 selects the fp32-MFMA kernels: its issued work is priced against the dense bf16 peak, the rest against the
        # fp32 peak, and `frac_issued` is the pipe time so priced over the measured time.
        flops_reg = 105216.0 * npix * B                     # 25.05 GFLOP per slice-step (direct form)
        flops1 = 2.0 * (F_hidden * 4 * 25 + F_hidden * F_hidden) * npix * B
        l1_bf16 = F_hidden == 64 and _lib.arith() != "fp32"
        l1_f16 = l1_bf16 and _lib.arith() == "f16x2"       # two-term fp16 operands: 66 MFMAs per 32 pixels instead of 132
        issued1_bf16 = ((66 if l1_f16 else 132) * 32 * 32 * 16 * 2 / 32.0) * npix * B if l1_bf16 else 0.0
        issued2_bf16 = executed if l2_bf16 else 0.0
        issued_l1_only = issued1_bf16             # layer 1's own bf16 MFMA work (for layer1_frac_issued)
        issued1_bf16 += issued2_bf16             # everything issued on the bf16 pipe
        issued_reg = flops_reg - (flops2 if l2_bf16 else flops2 - executed) - (flops1 if l1_bf16 else 0.0)      # fp32 part (none left with the final conv in layer 2's tail)
        pipe_ms = lambda f32, b16: 1e3 * (f32 / (PEAK_FP32_MFMA_TFLOPS * 1e12) + b16 / (PEAK_BF16_MFMA_TFLOPS * 1e12))  # noqa: E731
        final_flops = 0.0 if l2_taps else 2.0 * F_hidden * 2 * 9 * npix * B      # (in layer 2's launch when its tail does the contraction)
        issued_reg = max(issued_reg, 0.0)
        t_reg = (ms1 or 0) + (ms2 or 0) + (msf or 0)
        # tap planes layer 2 writes: 18, or 6 (+ 16 floats per row and 32-pixel tile) on the pre-summed route (ops.RIM_TAPS_Q: row-invariant masks at W = 372)
        tap_planes = 6.0 + 16.0 / 32.0 if (ops.RIM_TAPS_Q and args.mask == "1d" and W == 372 and ops.LLG372_GATHER) else 18.0
        roofline = dict(bound="mfma", kernel=kname,
                        achieved=tf(executed), peak=peak2, unit="TFLOP/s",
                        frac=(tf(executed) / peak2) if ms2 else None,
                        frac_meaning=("bf16 MFMA FLOPs the kernel issues (6 term products per fp32 multiply, padding included) / dense bf16 MFMA "
                                      "peak (pipe utilisation)" if l2_bf16 else "MFMA FLOPs the kernel issues / fp32-MFMA peak (pipe utilisation)"),
                        algorithmic_achieved=tf(flops2), algorithmic_frac=(tf(flops2) / PEAK_FP32_MFMA_TFLOPS) if ms2 else None,
                        algorithmic_note=("fp32 direct-form FLOPs of SURVEY 8d / time, against the fp32-MFMA peak: what the layer delivers in the units "
                                          "of the fp32 pipe it no longer uses (may exceed 1; not a pipe figure)" if l2_bf16 else
                                          "direct-form FLOPs of SURVEY 8d / time: above `frac` by the Winograd saving (2.0x), not a pipe figure"),
                        traffic=traffic.get("conv_layer2_f16" if l2_f16 else "conv_layer2_sb" if l2_bf16 else "conv_layer2_wino" if msw else "conv_layer2"), traffic_unit="bytes/launch",
                        traffic_kernel=traffic.get("_kernels", {}).get("conv_layer2_f16" if l2_f16 else "conv_layer2_sb" if l2_bf16 else "conv_layer2_wino" if msw else "conv_layer2"),
                        traffic_source=traffic.get("_source"), algorithmic_bytes=(3.0 * F_hidden + (tap_planes if l2_taps else 0.0)) * npix * B * 4,
                        # matrix-pipe utilisation by the hardware counters (committed PMC passes of this library version, like `traffic`):
                        # MFMA-pipe busy cycles / (4 SIMDs x CU busy cycles) -- independent of the clock the chip sustains under the kernel
                        # (bf16 MFMA kernels run at ~1.7-1.8 GHz here, `frac` prices the issued FLOPs against the 2.4 GHz peak)
                        mfma_util_pmc=traffic.get("_mfma_util", {}).get("conv_layer2_f16" if l2_f16 else "conv_layer2_sb" if l2_bf16 else "conv_layer2_wino" if msw else "conv_layer2"),
                        mfma_util_pmc_layer1=traffic.get("_mfma_util", {}).get("conv_layer1"),
                        mfma_util_pmc_regulariser=traffic.get("_mfma_util", {}).get("regulariser") if (l2_bf16 and l2_taps) else None,
                        mfma_util_pmc_source=traffic.get("_mfma_util_source"),
                        launches=n2, avg_ms=ms2, flops_per_launch=flops2, mfma_flops_per_launch=executed,
                        # (measured once per round, not live: profiles/r05_layer2_power_probe.txt, tools/probe/l2_power.py + l2_power_clock.py)
                        clock_note=("`peak` is the dense peak at 2.4 GHz.  This launch is granted 1.54 GHz (profiled) to ~1.8 GHz on full-entropy operands and 2.42 GHz on "
                                    "zero operands (same instruction stream, GRBM_GUI_ACTIVE / duration): time per slice = 69.5 k cycles / clock + 26 us of memory streams "
                                    "that do not scale with the clock (profiles/r05_layer2_power_probe.txt, r05_layer2_memory_ablation.txt)") if l2_f16 else None,
                        # the same launch against the HBM roofline (its algorithmic bytes: x, h_prev in, h_new and the tap planes out): with the
                        # two-term fp16 operands the kernel sits between its two bounds
                        hbm_frac=((3.0 * F_hidden + (tap_planes if l2_taps else 0.0)) * npix * B * 4 / (ms2 * 1e-3) / 1e9 / PEAK_HBM_GBS) if ms2 else None,
                        regulariser=dict(ms=t_reg, direct_form_gflop=flops_reg / 1e9, issued_fp32_gflop=issued_reg / 1e9,
                                         issued_bf16_gflop=issued1_bf16 / 1e9,
                                         frac_issued=(pipe_ms(issued_reg, issued1_bf16) / t_reg) if t_reg else None,
                                         note="all three kernels of a step: layer 1 and (unless MRIDC_AMD_ARITH=fp32: then fp32 MFMA, Winograd) layer 2 on "
                                              "the bf16 matrix pipe with fp32 results via the three-term split; final conv 64->2: its channel contraction in layer 2's tail on the "
                                              "matrix pipe + a 9-tap gather (default; the stand-alone vector-ALU kernel serves other shapes: its 0.55 GFLOP would count at the fp32 rate).  frac_issued = (fp32 work / fp32 peak + bf16 work / "
                                              "dense bf16 peak) / measured time",
                                         layer1_ms=ms1, layer1_kernel=("k_rim_layer1_sb<F16> (two fp16 terms per operand, per-unit / per-pixel scales, 3 term products)" if l1_f16 else
                                                        "k_rim_layer1_sb (three bf16 terms, 6 term products)") if l1_bf16 else "k_rim_layer<5,1,4>",
                                         layer1_frac_issued=(pipe_ms(0.0 if l1_bf16 else flops1, issued_l1_only) / ms1) if ms1 else None,
                                         layer1_hbm_frac=((2.0 * F_hidden + 8.0) * 4 * npix * B / (ms1 * 1e-3) / 1e9 / PEAK_HBM_GBS) if ms1 else None,   # h_prev in, h out, (eta, partial sums)
                                         # the two kernels that run on the matrix cores, on their own
                                         mfma_kernels_ms=(ms1 or 0) + (ms2 or 0),
                                         mfma_kernels_frac_issued=(pipe_ms(issued_reg - final_flops, issued1_bf16) / ((ms1 or 0) + (ms2 or 0)))
                                         if (ms1 and ms2) else None))
        bytes_llg = (25.0 + 16.0 * C) * npix * B     # compulsory bytes of one log_likelihood_gradient
        # the formulation executed for 1-D masks reads yt = IFFT_H(y) instead of y: the same (25+16C)N compulsory bytes per step
        # (plus one column pass per slice, outside the step, to make yt).  Since round 4 the data term is ONE constant plane per slice
        # (g = A^H M A eta - A^H M y: ops.LLG372_NO_Y / LLG_T4_NO_Y) and a step moves eta, S and the coil-group partial planes only:
        # `executed_bytes_per_call` / `executed_frac` price the launch on what it moves, `frac` on SURVEY 8d's figure for the operation
        no_y = bool(ms372 and getattr(ops, "LLG372_NO_Y", False)) or bool(args.mask != "1d" and getattr(ops, "LLG_T4_NO_Y", False))
        n_groups = -(-C // 5)
        bytes_llg_exec = ((8.0 + 8.0 * C + 8.0 * n_groups) * npix * B) if (no_y and ms372) else None
        roofline_fft = dict(bound="hbm", kernel=("mrx_llg372 (1-D column mask: H transforms cancel; ONE launch per step of wave-private prime-factor "
                                                 "12 x 31 row transforms on lane-ordered yt = IFFT_H(y), S and mask; coil-group sum finished by layer 1's "
                                                 "tile loader)" if ms372 else
                                                 "mrx_llg_hinv_parts (1-D column mask: H transforms cancel, ONE launch of row FFTs per step on "
                                                 "yt = IFFT_H(y), coil-chunk sum finished by layer 1's tile loader)" if args.mask == "1d"
                                                 else "mrx_llg (general mask: rows, columns + DC in LDS, rows: three launches)"),
                            achieved=(bytes_llg / (msl * 1e-3) / 1e9) if msl else None, peak=PEAK_HBM_GBS, unit="GB/s",
                            frac=(bytes_llg / (msl * 1e-3) / 1e9 / PEAK_HBM_GBS) if msl else None,
                            traffic=traffic.get("llg") if args.mask == "1d" else traffic.get("llg_2d"), traffic_unit="bytes/launch",
                            traffic_kernel=traffic.get("_kernels", {}).get("llg" if args.mask == "1d" else "llg_2d"),
                            launches=nl, avg_ms=msl, bytes_per_call=bytes_llg, executed_bytes_per_call=bytes_llg_exec,
                            # the same kernel with the previous step's nine-tap gather folded in (7 of 8 steps): its algorithmic bytes = the gradient's
                            # + the gather's (18 tap planes and eta in, eta out)
                            gather_form=(dict(kernel="k_llg372<0, true, true> via mrx_llg372_gather", launches=n372g, avg_ms=ms372g, traffic=traffic.get("llg_gather"),
                                              bytes_per_call=bytes_llg + 88.0 * npix * B,
                                              frac=((bytes_llg + 88.0 * npix * B) / (ms372g * 1e-3) / 1e9 / PEAK_HBM_GBS),
                                              executed_bytes_per_call=(bytes_llg_exec + 88.0 * npix * B) if bytes_llg_exec else None,
                                              executed_frac=((bytes_llg_exec + 88.0 * npix * B) / (ms372g * 1e-3) / 1e9 / PEAK_HBM_GBS) if bytes_llg_exec else None)
                                         if ms372g else None),
                            executed_frac=(bytes_llg_exec / (msl * 1e-3) / 1e9 / PEAK_HBM_GBS) if (msl and bytes_llg_exec) else None,
                            note=("`frac` = SURVEY 8d's compulsory bytes of the operation (eta, y, S, mask, result) / time; the launch itself does not read "
                                  "the measured data any more -- its term -A^H M y is a constant plane made once per slice -- and moves "
                                  "`executed_bytes_per_call` (eta, S, the coil-group partial planes): `executed_frac`.  The kernel is bound by its vector "
                                  "ALU work (two 31-point and six 12-point DFT passes per coil row, built without packed fp32), not by HBM."
                                  + ("  In the timed loop 7 of 8 launches per cascade are the form that first makes eta from the previous step's tap "
                                     "products (`gather_form`: k_llg372<0, true, true> in the rocprofv3 table, its bytes = this operation's + the gather's); "
                                     "this record is the plain launch k_llg372<0, true, false> (the first step of every cascade; the transform code is the same)"
                                     if ms372g else "")) if bytes_llg_exec else None)
        res = dict(metric=f"slices/sec (inference), CIRIM {cfg['num_cascades']}-cascade {C}-coil {H}x{W}"
                          + ("" if args.rnn == "IndRNN" else f" ({args.rnn})"), value=value, unit="slices/s",
                   n_gpus=world, steps=args.steps, warmup=args.warmup, ms_per_step=ms_per_step, higher_is_better=True,
                   scaling="weak", vs_baseline=None, dtype="f32", data="synthetic",
                   config=dict(workload=f"CIRIM {cfg['num_cascades']} cascades x {T_} time-steps ("
                                        + (f"config time_steps {cfg['time_steps']} rounded up as the reference does" if not args.rim_steps else
                                           f"--rim-steps: every block run as RIMBlock(time_steps={T_}) directly, no rounding") + f"), {args.rnn} {F_hidden} filters, "
                                        f"{C} coils, {H}x{W}, {NS * B} slice(s) per GPU and step ({NS} concurrent HIP stream(s) x batch {B}, "
                                        f"one hipGraph each), random-init weights (seed 0)",
                               global_batch=world * NS * B, streams_per_gpu=NS, coils=C, height=H, width=W, parallelism=f"slice-sharded x{world}",
                               mask=("1-D random columns R=4 (row-invariant: one-launch gradient)" if args.mask == "1d" else
                                     "2-D random points R~10 (general three-launch gradient)")),
                   world_size_seen=world_seen(), per_rank_ms_per_step=[1e3 * t / args.steps for t in per_rank],
                   numa_binding=NUMA_BINDING_ALL if NUMA_BINDING_ALL is not None else NUMA_BINDING,   # per rank: the NUMA node of its GPU and the CPUs it was restricted to (None: topology unreadable or its two sources disagree)
                   launch="hipGraph replay" if graphed else "eager", roofline=roofline, roofline_fft=roofline_fft,
                   breakdown_ms=dict(llg=llg_per_step, conv_layer1=ms1, conv_layer2=ms2, final=final_per_step,
                                     rim_steps_per_slice=cfg["num_cascades"] * T_,
                                     note=("per RIM step; llg = launches-weighted mean of the plain gradient launch and of the form that also forms eta from the "
                                           "previous step's tap products (mrx_llg372_gather); final = the stand-alone gather launches that remain (one per "
                                           "cascade) spread over the steps") if n372g else None),
                   event_timing=dict(method="HIP events around every launch of two eager steps (host enqueues ahead of a parked GPU); each figure "
                                            "is the event-pair time minus half an EMPTY pair, i.e. minus the closing event's own processing time, "
                                            "calibrated in this run -- this is what makes the figures agree with rocprofv3's kernel durations",
                                     empty_pair_ms=getattr(timer, "pair_ms", None),
                                     raw_ms=dict(llg=timer.raw_ms("llg372") or timer.raw_ms("llg"), conv_layer1=timer.raw_ms("conv_layer1"),
                                                 conv_layer2=timer.raw_ms("conv_layer2_f16t") or timer.raw_ms("conv_layer2_sbt") or timer.raw_ms("conv_layer2_sb") or timer.raw_ms("conv_layer2_wino") or timer.raw_ms("conv_layer2"),
                                                 final=timer.raw_ms("final_gather") or timer.raw_ms("final"))))
        if args.full:
            res["concurrent_replays_bit_identical_to_serial"] = headline_conc_ok
        else:                                   # a plain run recorded no per-kernel events: no roofline / breakdown records on its line
            for k_ in ("roofline", "roofline_fft", "breakdown_ms", "event_timing"):
                res.pop(k_)
        res["config"]["arith"] = ("fp32 tensors and fp32 accumulation; the two RIM layers multiply two-term fp16 operands (x = (h1 + h2) 2^-k, 22 significant "
                                  "bits, block-scaled by powers of two; three of the four term products) on v_mfma_f32_32x32x16_f16: error against float64 "
                                  "equal to the fp32-MFMA kernels' (2e-7); FFT / data consistency in fp32 vector arithmetic")
        if args.full and world == 1 and not args.no_other_configs:
            res["exact_fp32_route"] = exact_route_line(args)
        if args.full and world == 1 and args.stream_inputs:
            res["streamed_inputs"] = streamed_inputs_run(args, step, hosts, datas, dev, NS * B)
            if os.environ.get("MRX_BENCH_STREAM_PROBE"):     # which part of the streamed loop costs what (upload, staging copy, event wait)
                for v in ("no_h2d", "no_d2d", "no_wait", "full"):
                    print("[stream probe]", v, round(streamed_inputs_run(args, step, hosts, datas, dev, NS * B, variant=v)["value"], 2), file=sys.stderr)
        if args.full and world == 1 and not args.no_cpu_baseline:
            n_cpu = args.cpu_cascades if 0 < args.cpu_cascades <= cfg["num_cascades"] else cfg["num_cascades"]
            try:
                host1 = {k: v[:1] if k != "mask" else v for k, v in host.items()}
                cb, ref = cpu_baseline(cfg, state_dict, host1, n_cpu, args.cpu_slices)
                res["cpu_baseline"] = cb
                res["parity_vs_oracle"] = parity_vs_oracle(out[n_cpu - 1][-1][0:1], ref[n_cpu - 1][-1][0:1], host1["target"],
                                                           at=f"cascade {n_cpu} of {cfg['num_cascades']}, last time-step"
                                                              + (" (the final image)" if n_cpu == cfg["num_cascades"] else ""))
            except Exception as ex:  # noqa: BLE001
                res["cpu_baseline"] = dict(value=None, unit="slices/s", cores=os.cpu_count(), kind="port",
                                           sample=f"failed: {type(ex).__name__}: {ex}")
        if args.full and world == 1 and not args.no_other_configs:
            # BASELINE.json configs 1, 3, 4 next to the headline, each with its own roofline / cpu_baseline / parity records (short runs:
            # the driver times this whole process)
            del model, datas, data
            torch.cuda.empty_cache()
            import copy
            others = {}
            for name, fn, over in (("e2evn_6cascade_15coil_640x372", bench_e2evn, dict(model="e2evn", batch=8, streams=2, steps=6, warmup=2)),
                                   ("e2evn_precision16_15coil_640x372", bench_e2evn, dict(model="e2evn", batch=8, streams=2, steps=6, warmup=2, precision=16, cpu_slices=1)),
                                   ("qcirim_4echo_32coil_256x256", bench_qcirim, dict(model="qcirim", batch=1, streams=6, steps=10, warmup=2)),     # (streams 4 / 6 / 8: 740 / 790 / 781 slices/s, tools/runs/r06x.sh)
                                   ("qcirim_precision16_4echo_32coil_256x256", bench_qcirim, dict(model="qcirim", batch=1, streams=6, steps=10, warmup=2, precision=16, cpu_slices=1))):
                a2 = copy.copy(args)
                a2.dump_outputs = None                  # (the headline's outputs only)
                for k_, v_ in over.items():
                    setattr(a2, k_, v_)
                try:
                    r2 = fn(a2, world, rank, dev, checks=not args.no_cpu_baseline)
                    for drop in ("n_gpus", "higher_is_better", "scaling", "vs_baseline", "world_size_seen", "per_rank_ms_per_step", "data"):
                        r2.pop(drop, None)
                    others[name] = r2
                except Exception as ex:  # noqa: BLE001
                    others[name] = dict(value=None, error=f"{type(ex).__name__}: {ex}")
                torch.cuda.empty_cache()
            others["cirim_training_bf16_15coil_640x372"] = training_line(args)
            others["e2evn_training_15coil_640x372"] = training_line(args, "e2evn")
            from mridc_amd import autograd as ag_
            ag_.set_precision("f32")
            if args.mask == "1d":
                others["cirim_precision16_15coil_640x372"] = precision16_line(args)
                others["cirim_2d_mask_15coil_640x372"] = mask2d_line(args)
            if not args.rim_steps:
                others["cirim_8cascade_x5_time_steps_rimblock_direct"] = rim5_line(args)
            res["other_configs"] = others
        res["summary"] = summary_of(res)       # LAST key: the driver keeps the tail of this line
        emit(res)
    if use_dist:
        import torch.distributed as dist
        dist.destroy_process_group()
    flush_result()


if __name__ == "__main__":
    main()
