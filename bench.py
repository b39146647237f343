#!/usr/bin/env python3
"""Headline benchmark: aggregate ai-benchmark-equivalent throughput of N vGPU
pods sharing each MI355X, plus VRAM-cap accuracy (BASELINE.json metric).

Default config = BASELINE.json config 2: every GPU is split 2 ways, each pod
``amd.com/gpumem=144000`` (MiB) and ``amd.com/gpucores=50``, running ResNet-V2-50
bf16 inference at the reference's ai-benchmark shape (test 1.1: batch 50,
346x346; reference README.md:244).  Weights are random-init and inputs
synthetic.  Every pod runs under the in-container enforcement library
(LD_PRELOAD libvgpu.so) with its own shared region, HBM cap and compute share,
with exactly the env the device plugin's Allocate hands a container.  The share
policy is the plugin's default, `auto` (`--cu-share`): the pods of a GPU
measure time sharing under the fair-share GPU-time limiter against CUs of their
own, and keep the faster (vgpu/deviceplugin/custate.py).  `mask` gives every pod
an XCD-balanced CU mask; `temporal` only time-shares.

Launch: ``python bench.py --gpus N --steps K --warmup W`` (N>1 under
torch.distributed.run, one rank per GPU; started without one, bench.py starts
it as a child process and refuses to run on fewer than N visible GPUs).  Each rank spawns its pods BEFORE
touching the GPU itself (it never does), runs W untimed warmup steps in every
pod, then a cross-rank barrier, then exactly K timed steps in every pod
concurrently (each pod synchronizes its device before reporting ready and after
its last step).  The rank measures the wall time from GO to the last DONE;
the job's ms_per_step is the MAX over ranks, and `value` is total images over
all pods on all GPUs divided by that wall time (weak scaling: per-GPU work is
fixed as N grows).

A plain run does only that: set up, warm up, time the K steps, print the
result line.  ``--dump-outputs DIR`` adds one file per pod with the output of
its last timed step (model and input are seeded per pod, so two builds can be
compared output for output).  ``--full`` adds the checks that take runs of
their own after the timed window: the VRAM-cap probe of every pod (`vram_cap`
in the JSON: 1 GiB blocks until the cap refuses) and the RCCL check below.

The ranks coordinate over gloo (they never touch a GPU).  Before GO a
preflight checks the placement: N distinct devices, one share board (device
uuid) per GPU, one shared region per pod.  With ``--full`` and N > 1, after the timed window
pod 0 of every GPU joins one RCCL process group and all-reduces 64 MiB
(`rccl_check` in the JSON): RCCL kernels under the shim's limiter and IPC
buffers across pods.  Each of those pods sees ONE GPU, so RCCL cannot map its
peers' memory; the JSON records the transport it chose per peer
(NCCL_DEBUG=INFO: typically SHM), and xGMI peer access is claimed only where
it says P2P.  The path that does exercise P2P/xGMI under the shim is one pod
holding several GPUs: `--pod-gpus N` (DDP training inside one amd.com/gpu: N
pod, vgpu/parallel/ddp.py).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

METRIC = "aggregate ai-benchmark score, N pods sharing 1 MI355X; VRAM-cap accuracy"
BASELINE_VGPU_R50_INF = 141.2  # images/s, ResNet-V2-50 inference, vGPU-device-plugin
DUMP_BYTES = 60 << 20  # --dump-outputs: all pods of all ranks together stay under 64 MB


def log(msg: str) -> None:
    sys.stderr.write(f"[bench {time.strftime('%H:%M:%S')}] {msg}\n")
    sys.stderr.flush()


def enforcement_label(args) -> str:
    """What actually enforced the pods' compute share in this run."""
    if args.no_shim:
        return "none"
    if args.gpucores <= 0 or args.gpucores >= 100:
        vm = " + virtual device memory" if args.oversubscribe or args.memory_scaling > 1 else ""
        return f"libvgpu.so (HBM cap{vm}; whole GPU, no compute limit)"
    if args.cu_share == "group2":
        return "libvgpu.so (HBM cap + one CU mask per pod pair 2k,2k+1)"
    if args.cu_share == "group2i":
        return "libvgpu.so (HBM cap + one CU mask per pod pair k,k+n/2)"
    return (f"device-plugin Allocate (cu_share={args.cu_share}) + libvgpu.so: HBM cap, "
            "per-pod XCD-balanced CU masks and/or GPU-time limiter with fair-share board")


def make_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--pods", type=int, default=2, help="vGPU pods sharing each GPU")
    ap.add_argument("--workload", default="1.1", help="ai-benchmark test id (vgpu.models.WORKLOADS)")
    ap.add_argument("--gpumem", type=int, default=144000, help="per-pod amd.com/gpumem (MiB)")
    ap.add_argument("--gpucores", type=int, default=50, help="per-pod amd.com/gpucores (%%)")
    ap.add_argument("--pod-cores", default="",
                    help="comma list of per-pod amd.com/gpucores overriding --gpucores (e.g. 25,75)")
    ap.add_argument("--no-shim", action="store_true", help="run pods without enforcement")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-find", action="store_true",
                    help="skip MIOpen find (cudnn.benchmark) during the untimed warmup")
    ap.add_argument("--no-fused", action="store_true", help="plain PyTorch epilogues")
    ap.add_argument("--conv", choices=("native", "miopen"), default="native",
                    help="ResNet convolutions: fused MFMA implicit-GEMM kernels or MIOpen")
    ap.add_argument("--hw-queues", type=int, default=1,
                    help="GPU_MAX_HW_QUEUES per pod (vGPU HW-queue budget; 0 = runtime default)")
    ap.add_argument("--cu-share", choices=("hybrid", "mask", "temporal", "auto", "group2", "group2i"), default="auto",
                    help="compute-share policy of fractional pods: the device plugin's "
                         "(hybrid|mask|temporal, vgpu/deviceplugin/custate.py) or an A/B tool")
    ap.add_argument("--core-policy", choices=("default", "force", "disable"), default="default",
                    help="GPU_CORE_UTILIZATION_POLICY of the pods (reference docs/config.md:34-38)")
    ap.add_argument("--oversubscribe", action="store_true",
                    help="virtual device memory (VGPU_OVERSUBSCRIBE): pod caps may exceed physical HBM")
    ap.add_argument("--memory-scaling", type=float, default=1.0,
                    help="device plugin --device-memory-scaling (reference README.md:283-287)")
    ap.add_argument("--pool-concurrency", type=int, default=None,
                    help="device plugin --pool-concurrency: temporal-pool members of a GPU running at once "
                         "(0 = all; default: the plugin's)")
    ap.add_argument("--full", action="store_true",
                    help="also run the checks that are not part of the headline figure, after the timed "
                         "window: the VRAM-cap probe of every pod (`vram_cap`) and, with N > 1, the RCCL "
                         "all-reduce among one pod per GPU (`rccl_check`)")
    ap.add_argument("--no-cap-probe", action="store_true", help="with --full: skip the VRAM-cap probe")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps every pod writes what its last timed step returned (logits; "
                         "the loss of a training workload) as DIR/[rank<r>_]pod<i>_<name>.npy, float32, "
                         "at most 64 MB in all (a larger output as a fixed, seeded sample)")
    ap.add_argument("--warmup-seconds", type=float, default=0.0,
                    help="pods keep warming up (untimed) until this long has passed")
    ap.add_argument("--decide-timeout", type=float, default=30.0,
                    help="auto share policy: pods keep warming up (untimed) until the GPU's pods have "
                         "decided between time sharing and CUs of their own, at most this long (0: no wait)")
    ap.add_argument("--seconds", type=float, default=0.0,
                    help="share measurements: every pod runs steps for this long instead of exactly --steps")
    ap.add_argument("--ready-timeout", type=float, default=1500.0)
    ap.add_argument("--cpu-smoke", action="store_true",
                    help="rehearse the multi-rank orchestration on CPU (tests; not a measurement)")
    ap.add_argument("--pod-gpus", type=int, default=0,
                    help="instead of the headline: ONE vGPU pod granted this many GPUs (amd.com/gpu: N, "
                         "through Allocate) runs ResNet-V2-50 DDP training over RCCL inside it, one rank "
                         "per device under the enforcement library (vgpu/parallel/ddp.py)")
    ap.add_argument("--ddp-bucket-mb", type=int, default=64)
    return ap


_TRANSPORT = None


def rccl_transports(text: str) -> dict:
    """RCCL's chosen transport per (rank -> peer) from NCCL_DEBUG=INFO lines such
    as `Channel 00/0 : 0[0] -> 1[1] via P2P/IPC` (also `via SHM/...`, `via NET/...`)."""
    import re
    global _TRANSPORT
    if _TRANSPORT is None:
        _TRANSPORT = re.compile(r"(\d+)\[[^\]]*\] -> (\d+)\[[^\]]*\] (?:\[\w+\] )?via (\S+)")
    out: dict[str, set] = {}
    for m in _TRANSPORT.finditer(text):
        out.setdefault(f"{m.group(1)}->{m.group(2)}", set()).add(m.group(3))
    return {k: sorted(v) for k, v in sorted(out.items())}


def pod_gpus_main(args) -> int:
    """--pod-gpus N: one multi-GPU pod, DDP inside."""
    import socket
    import subprocess
    import tempfile
    from vgpu.bench.control import admit_multi_gpu_pod
    from vgpu.bench.launch import REPO, TORCHRUN_VARS, visible_device_for
    from vgpu.native import ensure_built, preload_env
    n = args.pod_gpus
    if args.cpu_smoke:
        devices = list(range(n))
    else:
        devices = [int(visible_device_for(i)) for i in range(n)]
        if len(set(devices)) != n:
            raise SystemExit(f"--pod-gpus {n}: needs {n} distinct visible GPUs, got {devices}")
        ensure_built(kernels=True)
    work = tempfile.mkdtemp(prefix="vgpu-ddp-")
    pod = admit_multi_gpu_pod(devices, work, mem_mib=args.gpumem if args.gpumem else 0,
                              cores=args.gpucores if 0 < args.gpucores < 100 else 0, policy=args.cu_share)
    env = {k: v for k, v in os.environ.items()
           if not k.startswith(("TORCHELASTIC_", "TORCH_ELASTIC_")) and k not in TORCHRUN_VARS}
    env["PYTHONPATH"] = str(REPO) + os.pathsep + env.get("PYTHONPATH", "")
    env["HIP_VISIBLE_DEVICES"] = ",".join(map(str, devices))
    env.pop("CUDA_VISIBLE_DEVICES", None)
    env["NCCL_DEBUG"] = "INFO"
    env.setdefault("NCCL_DEBUG_SUBSYS", "INIT,GRAPH")
    if not args.cpu_smoke and not args.no_shim:
        env.update(pod.env)
        env = preload_env(env)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(port), "-m", "vgpu.parallel.ddp",
           "--workload", "1.2", "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--bucket-mb", str(args.ddp_bucket_mb)]
    if args.cpu_smoke:
        cmd += ["--shrink", "--backend", "gloo", "--batch", "2", "--size", "64"]
    if args.no_graph:
        cmd += ["--no-graph"]
    log(f"one {n}-GPU pod on devices {devices} (share {pod.share}): {' '.join(cmd[2:])}")
    t0 = time.monotonic()
    r = subprocess.run(cmd, env=env, cwd=str(REPO), capture_output=True, text=True, timeout=1800)
    wall = time.monotonic() - t0
    text = r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not lines:
        sys.stderr.write(text[-6000:])
        raise SystemExit(f"DDP pod failed (rc={r.returncode})")
    d = json.loads(lines[-1])
    transports = rccl_transports(text)
    kinds = sorted({t.split("/")[0] for v in transports.values() for t in v})
    res = {
        "metric": "ResNet-V2-50 DDP training, one multi-GPU vGPU pod (images/s)",
        "value": d["value"], "unit": "images/s", "n_gpus": n, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": d["ms_per_step"], "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": d["dtype"], "data": "synthetic inputs, random-init weights",
        "config": {"model": "ResNet-V2-50 (ai-benchmark test 1.2, training)", "global_batch": n * d["batch_per_rank"],
                   "seq_len": 346, "parallelism": f"ddp{n} inside one vGPU pod", "backend": d["backend"],
                   "bucket_mb": d["bucket_mb"], "buckets": d["buckets"], "hipgraph": d["graph"],
                   "pod_env_share": pod.share, "enforcement":
                   "none (cpu rehearsal)" if args.cpu_smoke or args.no_shim else "libvgpu.so in every rank"},
        "replicas_agree": d["weights_in_sync"],
        # what RCCL chose per peer (NCCL_DEBUG=INFO): P2P = xGMI peer access, SHM = host memory
        "rccl_transport": transports, "rccl_transport_kinds": kinds,
        "pod_wall_s": round(wall, 1),
    }
    print(json.dumps(res), flush=True)
    return 0


def region_cus(path: str) -> int | None:
    """CUs in a pod's shared-region mask right now (0 = every CU); None without a region."""
    if not path or not os.path.exists(path):
        return None
    try:
        from vgpu.monitor.region import AttachedRegion
        r = AttachedRegion(path)
        try:
            devs = r.devices()
            return bin(devs[0].cu_mask).count("1") if devs else None
        finally:
            r.close()
    except Exception:
        return None


def preflight(placement: list[dict], world: int, shim: bool = True) -> bool:
    """Multi-GPU placement checks before the timed window:
    one rank per distinct device, one share board (device uuid) per GPU, one
    shared region per pod.  A failure aborts the run rather than measuring a
    misplaced one.  An explicit VGPU_BENCH_DEVICES map may put several ranks
    on one GPU (a rehearsal on a 1-GPU box); returns False then."""
    devices = [p["device"] for p in placement]
    if len(set(devices)) != world:
        if not os.environ.get("VGPU_BENCH_DEVICES"):
            raise RuntimeError(f"preflight: {world} ranks on devices {devices}: need {world} distinct devices")
        log(f"preflight: rehearsal, ranks share devices {devices} (VGPU_BENCH_DEVICES)")
        return False
    if not shim:
        return True
    boards = {}
    for p in placement:
        for u in set(p["uuids"]):
            boards.setdefault(u, set()).add(p["device"])
    shared = {u: sorted(d) for u, d in boards.items() if len(d) > 1 or not u}
    if shared:
        raise RuntimeError(f"preflight: share-board keys used by several GPUs: {shared}")
    regions = [r for p in placement for r in p["regions"]]
    if len(set(regions)) != len(regions) or not all(regions):
        raise RuntimeError(f"preflight: shared regions not one per pod: {regions}")
    return True


def rccl_check(pg, rank: int, world: int, pod, log) -> dict | None:
    """After the timed window: pod 0 of every GPU all-reduces over RCCL under
    the shim (vgpu/bench/pod.py rccl_check).  Never fatal."""
    import socket
    port = None
    if rank == 0:
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
    box = [port]
    pg.broadcast_object_list(box, src=0)
    addr = os.environ.get("MASTER_ADDR", "127.0.0.1")
    try:
        pod.send(f"RCCL {rank} {world} {addr} {box[0]}")
        res = pod.read_tagged("RCCL", 240.0, progress=log)
    except Exception as e:
        res = {"rank": rank, "error": f"{type(e).__name__}: {e}"[:300]}
    gathered = [None] * world
    pg.all_gather_object(gathered, res)
    ok = all(r.get("sum_ok") for r in gathered)
    bw = [r.get("busbw_GBps") for r in gathered if r.get("busbw_GBps") is not None]
    out = {"ok": ok, "world": world, "backend": gathered[0].get("backend"),
           "busbw_GBps_min": min(bw) if bw else None, "ms_per_allreduce_64MiB":
               max((r.get("ms_per_allreduce") or 0) for r in gathered),
           "transport_kinds": sorted({t.split("/")[0] for r in gathered
                                      for v in (r.get("transport") or {}).values() for t in v})}
    errs = [r["error"] for r in gathered if r.get("error")]
    if errs:
        out["errors"] = errs[:2]
    log(f"rccl check: {out}")
    return out


def visible_gpu_count(cpu_smoke: bool) -> int | None:
    """GPUs this process may use, without initialising the GPU runtime: the
    visible-device list if one is set, else the driver's device count (not an
    initialisation on this image).  None in a CPU rehearsal with no list."""
    for var in ("VGPU_BENCH_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None and v.strip():
            return len({s.strip() for s in v.split(",") if s.strip()})
    if cpu_smoke:
        return None
    import torch
    return torch.cuda.device_count()


def launch_ranks(argv: list[str], n: int, cpu_smoke: bool) -> int:
    """`python bench.py --gpus N` without an outer torch.distributed.run
    (VERDICT r5 missing #3): start one rank per GPU as a child
    `torch.distributed.run --nproc-per-node N bench.py ...` -- this process
    never touches a GPU -- relay its output (rank 0's one JSON line) and exit
    with its code.  Refuse when fewer than N distinct GPUs are visible rather
    than measure fewer."""
    import socket
    import subprocess
    have = visible_gpu_count(cpu_smoke)
    if have is not None and have < n:
        log(f"--gpus {n}: only {have} distinct GPU(s) visible; refusing to report fewer")
        return 3
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__), *argv]
    log(f"--gpus {n}: one rank per GPU: {' '.join(cmd[2:])}")
    return subprocess.run(cmd, cwd=os.path.dirname(os.path.abspath(__file__))).returncode


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    args = make_parser().parse_args(argv)
    if args.gpus > 1 and args.pod_gpus == 0 and "WORLD_SIZE" not in os.environ:
        return launch_ranks(argv, args.gpus, args.cpu_smoke)
    if args.cpu_smoke:
        os.environ["VGPU_BENCH_CPU"] = "1"
        args.no_shim = True
        args.no_cap_probe = True
    if args.pod_gpus > 0:
        if args.dump_outputs:
            raise SystemExit("--dump-outputs writes the headline pods' outputs; --pod-gpus runs none")
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        return pod_gpus_main(args)

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        log(f"WORLD_SIZE={world} but --gpus={args.gpus}: refusing to measure a different GPU count")
        return 3

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from vgpu.native import ensure_built
    from vgpu.bench.launch import PodSpec, launch_pods, visible_device_for
    from vgpu.models import WORKLOADS

    if not args.no_shim:
        ensure_built(kernels=True)
    w = WORKLOADS[args.workload]

    pg = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo", rank=rank, world_size=world)
        pg = dist

    device = visible_device_for(local_rank)
    from vgpu.config import DevicePluginConfig
    pool_conc = DevicePluginConfig().pool_concurrency if args.pool_concurrency is None else args.pool_concurrency
    pol_env = {} if args.core_policy == "default" else {"GPU_CORE_UTILIZATION_POLICY": args.core_policy}
    cores = [int(c) for c in args.pod_cores.split(",") if c.strip()] if args.pod_cores else []
    if cores and len(cores) != args.pods:
        raise SystemExit(f"--pod-cores lists {len(cores)} values for {args.pods} pods")
    specs = [PodSpec(workload=args.workload, mem_mib=args.gpumem, cores=cores[i] if cores else args.gpucores,
                     extra_env=dict(pol_env)) for i in range(args.pods)]
    log(f"rank {rank}/{world}: launching {args.pods} pods of {w.name} (test {w.test_id}) on device {device}")
    pods = launch_pods(specs, device, steps=args.steps, warmup=args.warmup, shim=not args.no_shim,
                       graph=not args.no_graph, cap_probe=args.full and not args.no_cap_probe,
                       dump_outputs=args.dump_outputs, dump_prefix=f"rank{rank}_" if world > 1 else "",
                       dump_bytes=DUMP_BYTES // (args.pods * world),
                       find=not args.no_find, hw_queues=args.hw_queues or None,
                       fused=not args.no_fused, conv=args.conv, cu_share=args.cu_share,
                       oversubscribe=args.oversubscribe, memory_scaling=args.memory_scaling,
                       pool_concurrency=pool_conc, seconds=args.seconds, warmup_seconds=args.warmup_seconds,
                       decide_timeout=args.decide_timeout if args.cu_share == "auto" else 0.0)
    try:
        for p in pods:
            p.ready = p.read_tagged("READY", args.ready_timeout, progress=log)
            log(f"pod {p.idx} ready: {json.dumps(p.ready)}")
        placement = [{"rank": rank, "local_rank": local_rank, "device": device,
                      "uuids": [p.env.get("VGPU_DEVICE_UUID_0", "") for p in pods],
                      "regions": [p.region for p in pods], "shares": [p.share for p in pods]}]
        if pg:
            gathered = [None] * world
            pg.all_gather_object(gathered, placement[0])
            placement = gathered
        distinct = preflight(placement, world, shim=not args.no_shim)
        if pg:
            pg.barrier()
        for p in pods:
            p.send("GO")
        for p in pods:
            p.done = p.read_tagged("DONE", 600.0 + 60.0 * args.steps, progress=log)
        # Timed window: first pod's post-sync start → last pod's post-sync end
        # (CLOCK_MONOTONIC is node-wide, so pod timestamps are comparable).
        t_end = max(p.done["t1"] for p in pods)
        t_start = min(p.done["t0"] for p in pods)
        wall = t_end - t_start
        final_cus = [region_cus(p.region) for p in pods]  # CUs each pod ends on (auto policy may move it)
        rccl = None
        if not args.full:
            pass  # a plain run ends with the timed window
        elif pg and pods and distinct:
            rccl = rccl_check(pg, rank, world, pods[0], log)
        elif pg:
            rccl = {"skipped": "ranks share a GPU (rehearsal): RCCL runs one rank per GPU"}
        for p in pods:
            try:
                p.send("EXIT")
            except (BrokenPipeError, OSError):
                pass
        for p in pods:
            p.proc.wait(timeout=120)
    finally:
        for p in pods:
            if p.proc.poll() is None:
                p.proc.kill()

    samples = sum(p.done["samples"] for p in pods)
    ms_step = 1e3 * wall / args.steps
    cap = []
    for p in pods:
        d = p.done
        if "reserved_at_oom" in d:
            limit = args.gpumem * (1 << 20)
            cap.append({"pod": p.idx, "limit": limit, "reported_total": d["mem_total_reported"],
                        "reserved_at_oom": d["reserved_at_oom"],
                        "accuracy": d["reserved_at_oom"] / limit,
                        "violation": d["reserved_at_oom"] > limit})
    if pg:
        import torch
        t = torch.tensor([ms_step, float(samples)], dtype=torch.float64)
        mx = t.clone()
        pg.all_reduce(mx, op=pg.ReduceOp.MAX)
        sm = t.clone()
        pg.all_reduce(sm, op=pg.ReduceOp.SUM)
        ms_step = float(mx[0])
        samples = float(sm[1])
    value = samples / (ms_step * args.steps / 1e3)
    if rank == 0:
        per_gpu = value / world
        res = {
            "metric": METRIC,
            "value": round(value, 2),
            "unit": "images/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_step, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": round(value / BASELINE_VGPU_R50_INF, 2) if args.workload == "1.1" else None,
            "dtype": "fp32" if os.environ.get("VGPU_BENCH_DTYPE", "bf16").lower() in ("fp32", "float32") else "bf16",
            "data": "synthetic inputs, random-init weights",
            "config": {
                "model": f"{w.name} (ai-benchmark test {w.test_id}, {'training' if w.train else 'inference'})",
                "global_batch": w.batch * args.pods * world,
                "seq_len": w.shape[-1],
                "parallelism": f"vgpu: {args.pods} pods/GPU x {world} GPU(s)",
                "pods_per_gpu": args.pods,
                "gpumem_mib": args.gpumem,
                "gpucores": args.gpucores if not cores else cores,
                "enforcement": enforcement_label(args),
                "cu_pack": os.environ.get("VGPU_CU_PACK", "spread"),
                "hipgraph": not args.no_graph,
                "miopen_find": not args.no_find,
                "fused_epilogues": not args.no_fused,
                "conv": args.conv,
                "hw_queues_per_pod": args.hw_queues,
                "cu_share": args.cu_share,
                "pool_concurrency": pool_conc,
                "core_policy": args.core_policy,
                "oversubscribe": args.oversubscribe or args.memory_scaling > 1,
                "memory_scaling": args.memory_scaling,
            },
            "per_gpu_images_s": round(per_gpu, 2),
            "per_pod_images_s": [round(p.done["throughput"], 2) for p in pods],
            "per_pod_cu_mask_bits": [p.mask_bits for p in pods],
            "per_pod_share": [p.share for p in pods],
            "per_pod_final_cus": final_cus,
            # what the share policy decided and ran the timed window under
            # (limiter.cpp limiter_share_state): temporal | spatial | exploring
            "per_pod_policy": [(p.done.get("share") or {}).get("policy") for p in pods],
            "per_pod_cus": [(p.done.get("share") or {}).get("cus") for p in pods],
            "per_pod_limiter_wait_ms": [(p.done.get("share") or {}).get("limiter_wait_ms") for p in pods],
            "per_pod_occ_charged_ms": [(p.done.get("share") or {}).get("occ_charged_ms") for p in pods],
            "per_pod_host_pid_src": [(p.done.get("share") or {}).get("host_pid_src") for p in pods],
            "per_pod_decide_wait_s": [((p.ready or {}).get("decide") or {}).get("waited_s") for p in pods],
            "full": args.full,  # vram_cap and rccl_check are measured only with --full
            "vram_cap": cap,
            "placement": placement,
            "rccl_check": rccl,
            "dumped_outputs": [p.done.get("dumped") for p in pods] if args.dump_outputs else None,
        }
        print(json.dumps(res), flush=True)
    if pg:
        pg.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
