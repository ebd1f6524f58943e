#!/usr/bin/env python3
"""Headline benchmark: truncated-EM E-step throughput of Binary Sparse Coding on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]

A "step" is one pass of the hot path -- select_Hprimes + E_step (prosper/em/camodels/
bsc_et.py:98-192) -- over one resident data shard of BASELINE config 2 per GPU:
D=1024, H=256, H'=8, gamma=4 (K = 411 truncated states), N = 200 000 datapoints per GPU,
synthetic BSC data generated on the device, float64 throughout.  Datapoints shard over ranks
with no data-path collective, so scaling is weak (config 3 = 8 x 200k = 1.6 M).

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times the K steps and prints the headline
(`value`, `ms_per_step`, the configuration, `per_rank`); `--dump-outputs DIR` also writes what the last timed step
returned (dump_outputs).  Everything below is measured with `--full` only.

The full EM iteration (CAModel.step incl. the one RCCL all-reduce and the H x H solve) is timed in a
second region and reported as `em_iter_ms`.  `roofline` prices the dominant kernel -- bsc_estep_fused_kernel: scores GEMM,
selection and E-step of 196 608 datapoints in one launch -- by its algorithmic flops / its average launch duration
measured with HIP events on its stream inside the timed region, and reports the whole pass against the MFMA and HBM
roofs beside it (`estep_mfma_frac`, `estep_hbm_frac`); `traffic` comes from committed PMC passes (`traffic_source`), the wave-instruction counts of the VALU-issue rooflines
likewise (`counts_source`, with `stale` = "taken on another build of the library").
`cpu_baseline` is the oracle's faithful per-datapoint restatement of the reference timed on this box's host cores on
a bounded sample (rank 0, N=1 only), with the rate of one uncontended process and of the oracle's vectorised
multi-threaded form beside it; `parity` compares the HIP path with the oracle's answer (minted by that same leg) after
3 EM steps on a seeded sample at the bench's dimensions -- outside every timed region; `per_rank` lists every rank's
own ms_per_step / em_iter_ms / all-reduce time / data seed; `other_models` adds the EM-iteration wall-clock, kernel
times and rooflines of GSC (config 4) and MCA (config 5), and the EM-iteration time of DSC and TSC, on this GPU, measured
after the headline (N=1 only;
`--no-other-models` skips it).
"""
import argparse
import gc
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

D, H, HP, GAMMA, N_PER_GPU = 1024, 256, 8, 4, 200_000
MFMA_F64_PEAK_TFLOPS = 78.6   # MI355X dense f64 matrix peak (datasheet; = 32 flop/clk/SIMD)
HBM_PEAK_GBS = 8000.0
DUMP_ROWS = 16384             # rows of the --dump-outputs sample: 16384 x 411 log-joints in f64 = 54 MB


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # defaults: the chip's clock ramps for ~35 ms of sustained load (scratch/gemm_clk.hip) and the first ~20 passes of a
    # process run 5-7 % slower than the steady state -- 25 untimed passes (50 ms) get past that, 50 timed ones
    # (100 ms) average over box jitter
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=25)
    ap.add_argument("--n-per-gpu", type=int, default=N_PER_GPU)
    ap.add_argument("--em-steps", type=int, default=20, help="full EM iterations timed for em_iter_ms")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-other-models", action="store_true", help="skip the GSC / MCA EM-iteration side measurements")
    ap.add_argument("--no-other-shapes", action="store_true", help="skip the E-step passes at off-config shapes")
    ap.add_argument("--cpu-budget", type=float, default=8.0)
    ap.add_argument("--prewarm-ms", type=float, default=150.0, help="untimed E-step passes by wall time before the warm-up")
    ap.add_argument("--backend", choices=("nccl", "gloo"), default="nccl",
                    help="process-group backend for --gpus > 1.  nccl (= RCCL over xGMI) is the product path; gloo is a "
                         "debugging switch that lets N ranks share whatever devices the box has (LOCAL_RANK modulo the "
                         "device count; RCCL refuses two ranks per device) -- tests/test_nccl_gpu.py runs the multi-rank "
                         "branch of this script end to end on the one-GPU box with it; never a SCALE measurement")
    ap.add_argument("--data", choices=("numpy", "device"), default="numpy",
                    help="numpy: SURVEY 8d's np.random.RandomState recipe (host draws, ~5 s); device: torch.Generator on the GPU")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: per-kernel times and rooflines, the EM-iteration loops (flat and on "
                         "the reference's schedule), the CPU baseline and parity, other models and shapes.  Without it the "
                         "run sets up, warms up, times --steps passes and prints the headline line")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed passes write what the last one returned to a caller as DIR/<name>.npy (rank 0): "
                         "the log-joints `logpj` and the `candidates` of a fixed, seeded sample of %d rows" % DUMP_ROWS)
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


VALU_COUNTS = "r06_valu_counts.json"
PMC_TRAFFIC = ("r06_pmc_traffic.json", "r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json", "r02_pmc_traffic.json", "r01_pmc_traffic.json")


def _library_sha16():
    import hashlib
    try:
        return hashlib.sha256(open(os.path.join(ROOT, "prosper_amd", "libprosper_hip.so"), "rb").read()).hexdigest()[:16]
    except OSError:
        return None


def valu_issue_roofline(kernel_prefix, measured_ms, what, grid=None):
    """Roofline of a VALU-bound row kernel against the f64 vector ISSUE roof: the kernel's dynamic wave-instruction count
    (SQ_INSTS_VALU per launch) x 4 cycles / (1024 SIMDs x 2.4 GHz) is the time the chip needs just to issue them; `frac` =
    that floor / the launch duration measured here.  The count is EXTERNAL evidence -- a separate rocprofv3 --pmc pass
    (profiles/r04_valu_counts.json, scratch/profile_r04.sh), not this run: `counts_library_sha16` is the build it was taken
    on and `stale` says whether that is the build running now (a kernel change moves the count: then the fraction is only
    indicative).  `grid`: the launch geometry to match when the file holds the kernel at several.
    (These kernels move a few hundred MB per launch: the HBM roof is 3-10x further away.)"""
    try:
        rec = json.load(open(os.path.join(ROOT, "profiles", VALU_COUNTS)))
        kern = rec["kernels"]
        key = [k for k in kern if k.startswith(kernel_prefix)]
        if grid is not None and any(k.endswith("@grid%d" % grid) for k in key):
            key = [k for k in key if k.endswith("@grid%d" % grid)]
        if not key:
            return None
        key = max(key, key=lambda k: kern[k]["valu_insts"])          # (the full-size launch, not a warm-up shape)
        insts = kern[key]["valu_insts"]
        floor_ms = insts * 4.0 / (1024 * 2.4e9) * 1e3
        sha = _library_sha16()
        return {"bound": "valu_issue", "kernel": what,
                "meaning": "pipe occupancy of THIS build's own instruction stream (wave-instructions x 4 cycles at 2.4 GHz over "
                           "the launch time) -- not an algorithmic roof: a leaner kernel lowers `achieved` and the time together",
                "achieved": insts / (measured_ms * 1e-3) / 1e9,
                "peak": 1024 * 2.4e9 / 4.0 / 1e9, "unit": "G wave-instructions/s", "frac": floor_ms / measured_ms,
                "avg_launch_ms": measured_ms, "issue_floor_ms": floor_ms, "valu_insts_per_launch": insts,
                "waves_per_launch": kern[key].get("waves"), "busy_cycles_per_launch": kern[key].get("busy_cycles"),
                "counts_source": "profiles/%s (%s; separate --pmc pass, not this run)" % (VALU_COUNTS, key),
                "counts_from_this_run": False, "counts_library_sha16": rec.get("library_sha16"),
                "stale": (rec.get("library_sha16") != sha) if (sha and rec.get("library_sha16")) else None,
                "traffic": None}
    except Exception as e:
        return {"error": repr(e)}


ANNEAL_STEPS = 50


def reference_schedule(steps=ANNEAL_STEPS):
    """The annealing schedule every shipped example of the reference runs (examples/barstests/bars-learning.py:77-80,
    the param-bars-*.py files, simple-barstest.py:64): T 2 -> 1 over the first 70 % of the steps, Ncut_factor 0 -> 1 over
    the first two thirds -- the annealing point moves on 35 of 50 steps and data truncation is on for 49 of them."""
    from prosper_amd.em.annealing import LinearAnnealing
    an = LinearAnnealing(steps)
    an['T'] = [(0, 2.), (.7, 1.)]
    an['Ncut_factor'] = [(0, 0.), (2. / 3, 1.)]
    an['anneal_prior'] = False
    return an


def annealed_em(model, params, data, steps=ANNEAL_STEPS, runs=2, barrier=None):
    """Wall-clock of the reference's own driver loop -- EM(model, anneal).run() (prosper/em/__init__.py:152-178) -- on
    `reference_schedule`, from `params`.  The first run is the warm-up (first-use allocations, cold inverse), the last one
    is timed; the split ramp (T still moving) / plateau comes from a time stamp at the entry of every model.step."""
    import torch
    from prosper_amd.em import EM
    out = {}
    stamps = []
    step = model.step

    def timed_step(anneal, p, d):
        stamps.append(time.perf_counter())
        return step(anneal, p, d)

    sync = barrier if barrier is not None else torch.cuda.synchronize
    model.step = timed_step
    try:
        for r in range(runs):
            an = reference_schedule(steps)
            em = EM(model=model, anneal=an, data=data, lparams={k: (v.copy() if hasattr(v, "copy") else v)
                                                                for k, v in params.items()})
            del stamps[:]
            hits0 = getattr(model, "spec_hits", 0) or 0
            sync()
            t0 = time.perf_counter()
            em.run()
            sync()
            t1 = time.perf_counter()
    finally:
        del model.step
    ramp = int(.7 * steps)                      # steps 0 .. ramp - 1 see a new temperature each
    edges = stamps + [t1]
    per = [(edges[i + 1] - edges[i]) * 1e3 for i in range(steps)]
    out["em_iter_annealed_ms"] = (t1 - t0) / steps * 1e3
    out["ramp_ms"] = sum(per[1:ramp]) / max(1, ramp - 1)             # (step 0 starts on an idle device)
    out["plateau_ms"] = sum(per[ramp:]) / max(1, steps - ramp)
    out["steps"] = steps
    out["schedule"] = "LinearAnnealing(%d): T [(0, 2.), (.7, 1.)], Ncut_factor [(0, 0.), (2/3, 1.)], anneal_prior False " \
                      "(bars-learning.py:77-80); EM.run wall-clock / steps, second of %d runs" % (steps, runs)
    out["spec_hits"] = (getattr(model, "spec_hits", 0) or 0) - hits0    # E-steps the previous M-step had already launched
    return out


def other_models(dev, Anneal, steps=20):
    """EM-iteration wall-clock of the other §8(a) models at BASELINE configs 4 and 5 (one GPU's share), after the
    headline timing: GSC D=256 H=128 H'=6 gamma=3 N=200k, MCA D=256 H=128 H'=8 gamma=3 N=100k.  Informational."""
    import gc
    import numpy as np
    import torch
    from prosper_amd.em.camodels.gsc_et import GSC
    from prosper_amd.em.camodels.mca_et import MCA_ET
    from prosper_amd.em.camodels._device import KernelTimer
    out = {}
    gc.collect()
    gc.disable()               # as in the headline loops: a full collection is a ~70-80 ms host stall
    try:
        Dm, Hm = 256, 128
        g = torch.Generator(device=dev).manual_seed(3)
        rng = np.random.RandomState(3)
        # --- GSC, config 4
        N = 200_000
        W_gt = torch.randn(Dm, Hm, generator=g, device=dev, dtype=torch.float64)
        Y = torch.empty(N, Dm, dtype=torch.float64, device=dev)
        for lo in range(0, N, 50_000):
            S = (torch.rand(50_000, Hm, generator=g, device=dev) < 2.0 / Hm).to(torch.float64)
            Z = S * (1.5 + torch.randn(50_000, Hm, generator=g, device=dev, dtype=torch.float64))
            Y[lo:lo + 50_000] = Z @ W_gt.t() + torch.randn(50_000, Dm, generator=g, device=dev, dtype=torch.float64)
        p = {"W": W_gt.cpu().numpy() + 0.1 * rng.normal(size=(Dm, Hm)), "pi": np.full(Hm, 2.0 / Hm),
             "mu": np.full(Hm, 1.4), "psi_sq": np.eye(Hm) * 1.1, "sigma_sq": 1.2}
        m = GSC(Dm, Hm, 6, 3, 'scalar')
        p0 = dict(p)
        t_warm = time.perf_counter()     # warm up by TIME: the HIP runtime stalls one asynchronous copy for ~80 ms
        while time.perf_counter() - t_warm < 0.5:   # once, 100-150 ms into a model's first EM loop
            p = m.step(Anneal(T=1.0), p, {"y": Y})
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(steps):
            p = m.step(Anneal(T=1.0), p, {"y": Y})
        torch.cuda.synchronize()
        out["gsc_c4_em_iter_ms"] = (time.perf_counter() - t) / steps * 1e3
        out["gsc_c4"] = "GSC D=256 H=128 H'=6 gamma=3 scalar sigma_sq, N=%d" % N
        out["gsc_c4_annealed"] = annealed_em(m, p0, {"y": Y})
        m.timer = kt = KernelTimer()
        for _ in range(3):
            p = m.step(Anneal(T=1.0), p, {"y": Y})
        m.timer = None
        ks = kt.summary()
        out["gsc_c4_kernels_ms"] = {k: round(v[1], 4) for k, v in sorted(ks.items())}
        if "estep" in ks:
            # dominant kernel: gsc_estep_kernel -- 35 multi-cause states with g x g solves in registers + 128 singletons per
            # datapoint: f64-VALU bound (not HBM: 3 H doubles per datapoint in and out, 0.6 GB per launch)
            out["gsc_c4_roofline"] = valu_issue_roofline("gsc_estep_kernel<8, 3, false,", ks["estep"][1],
                                                         "gsc_estep_kernel (select + E-step, one pass over the scores)")
            if out["gsc_c4_roofline"] and "frac" in out["gsc_c4_roofline"]:
                out["gsc_c4_roofline"]["note"] = (
                    "avg_launch_ms brackets the whole pm_gsc_estep_f64 call with HIP events: gsc_estep_kernel + "
                    "pm_fold_copies_kernel and the gap between the two launches; frac prices the call, i.e. reads a few "
                    "per cent low (the column-sum kernel of rounds 1-3 is gone: the sums are accumulated in the pass)")
        del Y, m
        # --- MCA, config 5 (N = 800k over 8 GPUs)
        N = 100_000
        W_gt = torch.randn(Dm, Hm, generator=g, device=dev, dtype=torch.float64).abs() * 2 + 0.1
        Y = torch.empty(N, Dm, dtype=torch.float64, device=dev)
        for lo in range(0, N, 25_000):
            S = torch.rand(25_000, Hm, generator=g, device=dev) < 2.0 / Hm
            Wm = torch.where(S[:, None, :], W_gt[None, :, :].expand(25_000, Dm, Hm),
                             torch.zeros((), dtype=torch.float64, device=dev)).max(dim=2).values
            Y[lo:lo + 25_000] = Wm + torch.randn(25_000, Dm, generator=g, device=dev, dtype=torch.float64)
        p = {"W": (W_gt * (1 + 0.1 * (2 * torch.rand(Dm, Hm, generator=g, device=dev, dtype=torch.float64) - 1))).cpu().numpy(),
             "pi": 2.0 / Hm, "sigma": 1.0}
        m = MCA_ET(Dm, Hm, 8, 3)
        p0 = dict(p)
        t_warm = time.perf_counter()     # warm up by TIME: the HIP runtime stalls one asynchronous copy for ~80 ms
        while time.perf_counter() - t_warm < 0.5:   # once, 100-150 ms into a model's first EM loop
            p = m.step(Anneal(T=1.0), p, {"y": Y})
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(steps):
            p = m.step(Anneal(T=1.0), p, {"y": Y})
        torch.cuda.synchronize()
        out["mca_c5_em_iter_ms"] = (time.perf_counter() - t) / steps * 1e3
        out["mca_c5"] = "MCA_ET D=256 H=128 H'=8 gamma=3, N=%d (one GPU's share of 800k)" % N
        out["mca_c5_annealed"] = annealed_em(m, p0, {"y": Y})
        m.timer = kt = KernelTimer()
        for _ in range(3):
            p = m.step(Anneal(T=1.0), p, {"y": Y})
        m.timer = None
        ks = kt.summary()
        out["mca_c5_kernels_ms"] = {k: round(v[1], 4) for k, v in sorted(ks.items())}
        lab = "estep_mstats" if "estep_mstats" in ks else ("estep" if "estep" in ks else None)
        if lab:
            # dominant kernel: the fused E-step + M-statistics pass: one f64 power per multi-cause state and observed
            # dimension (S x D per datapoint, 36 VALU issue slots each) + the state loop around it: f64-VALU bound
            out["mca_c5_roofline"] = valu_issue_roofline("mca_estep_fused_kernel<4, 8, false,", ks[lab][1],
                                                         "mca_estep_fused_kernel (E-step + M-step statistics)")
            r = out["mca_c5_roofline"]
            if r and "valu_insts_per_launch" in r:
                # per (multi-cause state, 64 observed dimensions): what the build issues against what the algebra needs --
                # the power 15 (round 6: pm_pow_uni, the uniform-exponent power at every rho; rounds 4-5: the rho = 21 root, 26)
                # + T sum <= 3 + energy 3 + V update ~4 + the state's reduction / exponential / weight ~30 / 4
                groups = N * 84 * (Dm // 64)
                r["insts_per_state_group"] = round(r["valu_insts_per_launch"] / groups, 1)
                r["algorithmic_min_insts_per_state_group"] = 32
                r["algorithmic_floor_ms"] = round(32 * groups * 4.0 / (1024 * 2.4e9) * 1e3, 3)
                r["algorithmic_floor_note"] = ("the floor moved with the algebra: 43 instructions per state group (2.35 ms) while the "
                                               "power was the rho = 21 root of rounds 4-5")
                r["frac_of_algorithmic_floor"] = round(r["algorithmic_floor_ms"] / ks[lab][1], 3)
        del m, Y
        # --- the "next" models of SURVEY 8(f2) on the same skeleton: DSC (ternary latents) and TSC, D=256 H=128 H'=6
        # gamma=3, N=100k (no BASELINE config names them; same shapes as configs 4 / 5)
        from prosper_amd.em.camodels.dsc_et import DSC_ET
        from prosper_amd.em.camodels.tsc_et import TSC_ET
        N = 100_000
        W_gt = torch.randn(Dm, Hm, generator=g, device=dev, dtype=torch.float64) * 2
        Y = torch.empty(N, Dm, dtype=torch.float64, device=dev)
        for lo in range(0, N, 25_000):
            u = torch.rand(25_000, Hm, generator=g, device=dev)
            S = (u < 1.0 / Hm).to(torch.float64) - (u > 1 - 1.0 / Hm).to(torch.float64)
            Y[lo:lo + 25_000] = S @ W_gt.t() + torch.randn(25_000, Dm, generator=g, device=dev, dtype=torch.float64)
        W0 = (W_gt + 0.1 * torch.randn(Dm, Hm, generator=g, device=dev, dtype=torch.float64)).cpu().numpy()
        from prosper_amd.em.camodels.mmca_et import MMCA_ET
        for name, m, p in (("dsc", DSC_ET(Dm, Hm, 6, 3, states=np.array([-1., 0., 1.])),
                            {"W": W0, "pi": np.array([1.0 / Hm, 1 - 2.0 / Hm, 1.0 / Hm]), "sigma": 1.0}),
                           ("tsc", TSC_ET(Dm, Hm, 6, 3), {"W": W0, "pi": 2.0 / Hm, "sigma": 1.0}),
                           # MMCA (signed max-superposition) on the same signed data at config-5 dimensions: H' = 8
                           ("mmca", MMCA_ET(Dm, Hm, 8, 3), {"W": W0, "pi": 2.0 / Hm, "sigma": 1.0})):
            p0 = dict(p)
            t_warm = time.perf_counter()
            while time.perf_counter() - t_warm < 0.3:
                p = m.step(Anneal(T=1.0), p, {"y": Y})
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(steps):
                p = m.step(Anneal(T=1.0), p, {"y": Y})
            torch.cuda.synchronize()
            out["%s_em_iter_ms" % name] = (time.perf_counter() - t) / steps * 1e3
            out[name] = "%s D=256 H=128 H'=%d gamma=3, N=%d" % (type(m).__name__, m.Hprime, N)
            out["%s_annealed" % name] = annealed_em(m, p0, {"y": Y})
            m.timer = kt = KernelTimer()
            for _ in range(3):
                p = m.step(Anneal(T=1.0), p, {"y": Y})
            m.timer = None
            ks = kt.summary()
            out["%s_kernels_ms" % name] = {k: round(v[1], 4) for k, v in sorted(ks.items())}
            if name == "dsc":       # (the DSC row kernel; TSC runs the same kernel on its own state table)
                if "estep_mstats" in ks:
                    out["dsc_estep_mstats_roofline"] = valu_issue_roofline(
                        "dsc_only:dsc_estep16_ms_kernel", ks["estep_mstats"][1],
                        "dsc_estep16_ms_kernel (log-joints of the K-ary states + the M-step's row statistics, one pass)")
    except Exception as e:   # never lose the headline over the side measurements
        out["error"] = repr(e)
    gc.enable()
    return out


OTHER_SHAPES = ((256, 128, 6, 3), (1024, 256, 6, 3), (1024, 256, 10, 4), (784, 400, 8, 3), (1024, 512, 8, 4), (4096, 1024, 10, 3))


def other_shapes(dev, Anneal, budget_s=40.0):
    """The E-step pass (the headline's estep_pass: new W^T installed, Gram + scores + selection + log-joints recomputed) at
    shapes the reference accepts (it asserts only H' <= H, gamma <= H': camodels/__init__.py:90-91) but no BASELINE config
    names -- datapoints/s, the fraction of the f64 MFMA roof the scores GEMM's flops amount to (2 D H per datapoint), the
    fraction of the HBM roof (SURVEY 8d's bytes: y, candidates, logpj) and WHICH code path the host layer took: only
    H in (128, 256], H' = 8, gamma in {3, 4} runs the tuned 16-wavefront kernel.  Also GSC with gamma = 4 and MCA with H' = 10
    (EM iteration).  N: 1.2 GB of data per shape at most.  Informational; tests/test_limits_gpu.py holds the same shapes
    to the oracle."""
    import gc
    import numpy as np
    import torch
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels._device import KernelTimer
    out, t_start = [], time.perf_counter()
    gc.collect()
    for (D, H, Hp, gamma) in OTHER_SHAPES:
        rec = {"model": "BSC_ET", "D": D, "H": H, "Hprime": Hp, "gamma": gamma}
        try:
            if time.perf_counter() - t_start > budget_s:
                rec["skipped"] = "time budget"
                out.append(rec)
                continue
            # whole rounds of 128-row tiles on 256 CUs (32768 datapoints): what a large shard amounts to -- a ragged last
            # round costs every tiled kernel a whole tile time (config 2's own N = 200 000 is 6.1 rounds; rounds 4-5 used
            # multiples of 1024 here and timed 4.47 rounds as 5 on the one-kernel paths)
            N = int(min(200_000, 1.2e9 / (8 * D)) // 32768 * 32768)
            g = torch.Generator(device=dev).manual_seed(0)
            W_gt = torch.randn(D, H, generator=g, device=dev, dtype=torch.float64)
            Y = torch.empty(N, D, dtype=torch.float64, device=dev)
            for lo in range(0, N, 25_000):
                n = min(25_000, N - lo)
                S = (torch.rand(n, H, generator=g, device=dev) < 4.0 / H).to(torch.float64)
                Y[lo:lo + n] = S @ W_gt.t() + torch.randn(n, D, generator=g, device=dev, dtype=torch.float64)
            Wt_dev = (W_gt + 0.1 * torch.randn(D, H, generator=g, device=dev, dtype=torch.float64)).t().contiguous()
            Wt_host = Wt_dev.cpu().numpy()
            params = {"W": Wt_host.T, "pi": 4.0 / H, "sigma": 1.0}
            m = BSC_ET(D, H, Hp, gamma)
            data, an = {"y": Y}, Anneal(T=1.0)

            def estep_pass():
                m.install_parameters(data, Wt_dev, Wt_host)
                return m.E_step(an, params, m.select_Hprimes(params, data))
            tw = time.perf_counter()
            while time.perf_counter() - tw < 0.25:
                estep_pass()
                torch.cuda.synchronize()
            gc.disable()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                estep_pass()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / 10 * 1e3
            gc.enable()
            m.timer = kt = KernelTimer()
            for _ in range(2):
                estep_pass()
            m.timer = None
            ks = {k: round(v[1], 4) for k, v in kt.summary().items()}
            K = 1 + H + m.no_states
            dps = N / (ms * 1e-3)
            rec.update({"N": N, "K": K, "ms_per_pass": round(ms, 4), "dp_per_s": round(dps),
                        "estep_mfma_frac": round(dps * 2 * D * H / 78.6e12, 4),
                        "estep_hbm_frac": round(dps * (8 * D + 4 * Hp + 8 * K) / 8e12, 4),
                        "path": ("one kernel, 16-wavefront tile (bsc_fused8.hip)" if (m._fused() and m._tile8_whole_shard()) else
                                 "one kernel, 4-wavefront tile (bsc_fused.hip)" if m._fused() else
                                 "scores GEMM + 16-lane row kernel (bsc_rows16.hip)" if "select_estep" in ks else
                                 "scores GEMM + select + E-step kernels (bsc_kernels.hip)"),
                        "kernels_ms": ks})
            del Y, m
            torch.cuda.empty_cache()
        except Exception as e:
            rec["error"] = repr(e)[:300]
        out.append(rec)
    # --- GSC with gamma = 4 (g x g systems in registers: one wavefront per SIMD), MCA with H' = 10: EM iterations
    try:
        from prosper_amd.em.camodels.gsc_et import GSC
        from prosper_amd.em.camodels.mca_et import MCA_ET
        Dm, Hm = 256, 128
        g = torch.Generator(device=dev).manual_seed(5)
        rng = np.random.RandomState(5)
        for name, N in (("gsc", 100_000), ("mca", 50_000)):
            if time.perf_counter() - t_start > budget_s + 15.0:
                out.append({"model": name, "skipped": "time budget"})
                continue
            W_gt = torch.randn(Dm, Hm, generator=g, device=dev, dtype=torch.float64)
            Y = torch.empty(N, Dm, dtype=torch.float64, device=dev)
            if name == "gsc":
                for lo in range(0, N, 25_000):
                    S = (torch.rand(25_000, Hm, generator=g, device=dev) < 2.0 / Hm).to(torch.float64)
                    Z = S * (1.5 + torch.randn(25_000, Hm, generator=g, device=dev, dtype=torch.float64))
                    Y[lo:lo + 25_000] = Z @ W_gt.t() + torch.randn(25_000, Dm, generator=g, device=dev, dtype=torch.float64)
                p = {"W": W_gt.cpu().numpy() + 0.1 * rng.normal(size=(Dm, Hm)), "pi": np.full(Hm, 2.0 / Hm),
                     "mu": np.full(Hm, 1.4), "psi_sq": np.eye(Hm) * 1.1, "sigma_sq": 1.2}
                m, what = GSC(Dm, Hm, 6, 4, 'scalar'), "GSC D=256 H=128 H'=6 gamma=4"
            else:
                W_gt = W_gt.abs() * 2 + 0.1
                for lo in range(0, N, 25_000):
                    S = torch.rand(25_000, Hm, generator=g, device=dev) < 2.0 / Hm
                    Wm = torch.where(S[:, None, :], W_gt[None, :, :].expand(25_000, Dm, Hm),
                                     torch.zeros((), dtype=torch.float64, device=dev)).max(dim=2).values
                    Y[lo:lo + 25_000] = Wm + torch.randn(25_000, Dm, generator=g, device=dev, dtype=torch.float64)
                p = {"W": (W_gt * 1.05).cpu().numpy(), "pi": 2.0 / Hm, "sigma": 1.0}
                m, what = MCA_ET(Dm, Hm, 10, 3), "MCA_ET D=256 H=128 H'=10 gamma=3"
            tw = time.perf_counter()
            while time.perf_counter() - tw < 0.3:
                p = m.step(Anneal(T=1.0), p, {"y": Y})
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                p = m.step(Anneal(T=1.0), p, {"y": Y})
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / 10 * 1e3
            m.timer = kt = KernelTimer()
            for _ in range(2):
                p = m.step(Anneal(T=1.0), p, {"y": Y})
            m.timer = None
            out.append({"model": what, "N": N, "em_iter_ms": round(ms, 4), "dp_per_s_em": round(N / (ms * 1e-3)),
                        "kernels_ms": {k: round(v[1], 4) for k, v in sorted(kt.summary().items())}})
            del Y, m
            torch.cuda.empty_cache()
    except Exception as e:
        out.append({"model": "gsc/mca", "error": repr(e)[:300]})
    gc.enable()
    return out


PARITY_FILE = os.path.join(tempfile.gettempdir(), "prosper_amd_parity_%d.npz" % os.getpid())


def parity_report(model_cls, anneal_cls):
    """SURVEY 8d "parity check reported with the numbers": the oracle's answer (written by the cpu_baseline
    leg as plain arrays) against the HIP path on the same seeded sample at the bench's dimensions."""
    import numpy as np
    if not os.path.exists(PARITY_FILE):
        return None
    try:
        ref = np.load(PARITY_FILE)
        m = model_cls(D, H, HP, GAMMA)
        p = {"W": ref["W0"].copy(), "pi": float(ref["pi0"]), "sigma": float(ref["sigma0"]), "mu": np.zeros(D)}
        data = {"y": ref["y"]}
        steps = int(ref["steps"])
        cand_same = None
        for k in range(steps):
            if k == 0:
                cand = np.asarray(m.select_Hprimes(p, dict(data))["candidates"])
                cand_same = float((np.sort(cand, 1) == np.sort(ref["candidates1"], 1)).all(axis=1).mean())
            p = m.step(anneal_cls(T=1.0), p, data)
        rel = lambda a, b: float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))
        return {"sample": "%d datapoints at the bench's dimensions, %d EM steps, oracle (vectorised NumPy restatement, "
                          "golden-pinned) vs HIP path" % (ref["y"].shape[0], steps),
                "W_rel_frobenius": rel(p["W"], ref["W"]), "pi_rel": abs(p["pi"] / float(ref["pi"]) - 1.0),
                "sigma_rel": abs(p["sigma"] / float(ref["sigma"]) - 1.0),
                "candidate_sets_identical_frac": cand_same, "tolerance": 1e-4}
    except Exception as e:   # never lose the measurement over the report
        return {"error": repr(e)}
    finally:
        try:
            os.remove(PARITY_FILE)
        except OSError:
            pass


def dump_outputs(out_dir, data, result):
    """--dump-outputs: what the last timed pass handed its caller -- ``data['candidates']`` from select_Hprimes and the
    log-joints ``logpj`` from E_step -- on the rows of a fixed sample (RandomState(0), sorted), gathered on the device.
    The inputs are seeded, so two builds run with the same arguments can be compared array for array."""
    import numpy as np
    import torch
    logpj, cand = result["logpj"].tensor, data["candidates"].tensor
    N = logpj.shape[0]
    rows = np.sort(np.random.RandomState(0).choice(N, min(N, DUMP_ROWS), replace=False))
    idx = torch.from_numpy(rows).to(logpj.device)
    os.makedirs(out_dir, exist_ok=True)
    for name, t in (("logpj", logpj), ("candidates", cand)):
        np.save(os.path.join(out_dir, name + ".npy"), t.index_select(0, idx).to(torch.float64).cpu().numpy())


def cpu_baseline(args):
    """Oracle leg, run as a child process BEFORE this process touches the GPU."""
    cmd = [sys.executable, os.path.join(ROOT, "oracle", "cpu_baseline.py"), "--D", str(D), "--H", str(H),
           "--Hprime", str(HP), "--gamma", str(GAMMA), "--budget", str(args.cpu_budget),
           "--full-budget", str(min(6.0, args.cpu_budget)), "--solo-budget", "3", "--vec-budget", "3",
           "--parity-out", PARITY_FILE]
    # the child is plain NumPy: keep profiler / tool injection (rocprofv3 preloads its library into every
    # descendant) out of its 100+ worker processes
    env = {k: v for k, v in os.environ.items()
           if k != "LD_PRELOAD" and not k.startswith(("ROCP", "ROCPROF", "HSA_TOOLS", "ROCTRACER", "ROCTX"))}
    try:
        out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=240,
                             env=env).stdout.strip().splitlines()
        return json.loads(out[-1])
    except Exception as e:  # the GPU numbers are still worth printing
        return {"value": None, "unit": "datapoints/s", "cores": 0, "kind": "port", "sample": "failed: %r" % (e,)}


def gather_per_rank(mine, world, backend, comm):
    """Every rank's record (a 1-D float64 tensor on its device) as rows of one array, on every rank."""
    import numpy as np
    import torch
    import torch.distributed as dist
    if world == 1:
        return mine.cpu().numpy()[None, :]
    if backend == "nccl":
        allr = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        return torch.stack(allr).cpu().numpy()
    return np.stack(comm.allgather(mine.cpu().numpy()))


def headline(args, world, N, elapsed, prewarm_ms):
    """The keys of the result line that a plain run prints: the timed E-step passes (`elapsed`: the slowest rank's)."""
    return {
        "metric": "E-step datapoints/sec (+ EM-iter wall-clock) BSC D=1024 H=256 H'=8",
        "value": world * N * args.steps / elapsed, "unit": "datapoints/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "prewarm_ms": prewarm_ms,
        "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f64", "data": "synthetic" if args.data == "device" else "synthetic (np.random.RandomState recipe of SURVEY 8d: W_gt seed 0, rows of rank r seed r)",
        "config": {"workload": "BSC_ET synthetic Gaussian D=1024 H=256 H'=8 gamma=4 (K=411 states), "
                               "N=%d datapoints per GPU, select_Hprimes+E_step per step" % N,
                   "global_datapoints": world * N, "parallelism": "dp%d" % world,
                   "backend": ("rccl" if args.backend == "nccl" else "gloo (debug: ranks may share a device)")
                              if world > 1 else None},
    }


def main():
    args = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and world == 1:
        # convenience: self-launch one rank per GPU (child process; nothing here touched the GPU yet)
        port = os.environ.get("MASTER_PORT", "29531")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", port, os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.run(cmd).returncode)         # (children start fresh: this process never touched the GPU)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))

    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline(args)

    import numpy as np
    import torch
    import torch.distributed as dist
    from prosper_amd.em.camodels.bsc_et import BSC_ET, KernelTimer
    from prosper_amd.utils import parallel

    shared_devices = world > 1 and args.backend == "gloo"
    if shared_devices:
        local_rank %= max(1, torch.cuda.device_count())
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group("gloo")
    comm = parallel.Comm()
    comm.time_collectives(True)
    # self-check of the launch (a SCALE record must be attributable): the process group has as many ranks as --gpus asks
    # for, every rank sits on its own device
    assert comm.size == world == max(1, args.gpus), "--gpus %d but WORLD_SIZE / process group say %d / %d" % (
        args.gpus, world, comm.size)
    if world > 1:
        devs = comm.allgather((rank, local_rank, torch.cuda.current_device()))
        assert sorted(d[0] for d in devs) == list(range(world)), devs
        assert shared_devices or len({d[2] for d in devs}) == world, devs

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # ---- synthetic workload: same W_gt everywhere, rank-seeded rows
    N = args.n_per_gpu
    Y = torch.empty(N, D, dtype=torch.float64, device=dev)
    if args.data == "numpy":
        # the survey's recipe: np.random.RandomState(0) -> W_gt = randn(D, H), start W = W_gt + 0.1 randn; rows of rank r
        # from RandomState(r) in the reference generator's order (latents, then noise: camodels/__init__.py:119-120,
        # bsc_et.py:92); the products run on the device
        rs0 = np.random.RandomState(0)
        W_gt_h = rs0.randn(D, H)
        W0 = np.ascontiguousarray((W_gt_h + 0.1 * rs0.randn(D, H)).T).T
        W_gt = torch.from_numpy(W_gt_h).to(dev)
        data_seed = rank
        rs = np.random.RandomState(data_seed)
        for lo in range(0, N, 25_000):
            hi = min(N, lo + 25_000)
            S = torch.from_numpy((rs.random_sample((hi - lo, H)) < 4.0 / H).astype(np.float64)).to(dev)
            noise = torch.from_numpy(rs.normal(size=(hi - lo, D))).to(dev)
            Y[lo:hi] = torch.addmm(noise, S, W_gt.t())
        del noise
    else:
        g0 = torch.Generator(device=dev).manual_seed(0)
        W_gt = torch.randn(D, H, generator=g0, device=dev, dtype=torch.float64)
        # (D,H) parameter matrix laid out as an M-step returns it: the transposed view of a C-contiguous (H,D) array
        W0 = np.ascontiguousarray((W_gt + 0.1 * torch.randn(D, H, generator=g0, device=dev, dtype=torch.float64)).cpu().numpy().T).T
        data_seed = 100 + rank
        gr = torch.Generator(device=dev).manual_seed(data_seed)
        for lo in range(0, N, 25_000):      # chunked so the generator temporaries stay small
            hi = min(N, lo + 25_000)
            S = (torch.rand(hi - lo, H, generator=gr, device=dev) < 4.0 / H).to(torch.float64)
            Y[lo:hi] = S @ W_gt.t() + torch.randn(hi - lo, D, generator=gr, device=dev, dtype=torch.float64)
    del S
    params = {"W": W0, "pi": 4.0 / H, "sigma": 1.0, "mu": np.zeros(D)}

    class Anneal(dict):
        crit_params = []

        def __missing__(self, k):
            return 0.0

        def as_dict(self):
            return dict(self)

    anneal = Anneal(T=1.0, Ncut_factor=0.0, anneal_prior=False)
    model = BSC_ET(D, H, HP, GAMMA, comm=comm)
    data = {"y": Y}

    Wt_host = np.ascontiguousarray(W0.T)
    Wt_dev = torch.from_numpy(Wt_host).to(dev)

    def estep_pass():
        # steady state of an EM loop (parameters resident): W^T is on the device, as the M-step leaves
        # it, and it is NEW every step -- the Gram matrix and every score are recomputed in each pass
        model.install_parameters(data, Wt_dev, Wt_host)
        d = model.select_Hprimes(params, data)
        return model.E_step(anneal, params, d)

    # Pre-warm by TIME (disclosed as prewarm_ms): the chip needs ~35 ms of sustained load to reach the clock it then
    # holds and the first ~20 passes of a process run 5-7 % slow; without this a short run (--steps 20 --warmup 5 is a
    # 40 ms timed region) would be measured inside the ramp.  Then the W counted warm-up passes, then the K timed ones.
    gc.collect()
    gc.disable()           # a full collection of a torch process is a ~70 ms host stall (an idle GPU drops its clock): none
    torch.cuda.synchronize()   # between here and the end of the timed loop
    tw = time.perf_counter()
    while time.perf_counter() - tw < args.prewarm_ms * 1e-3:
        for _ in range(5):
            estep_pass()
        torch.cuda.synchronize()
    prewarm_ms = (time.perf_counter() - tw) * 1e3
    for _ in range(args.warmup):
        estep_pass()
    # --full: HIP events around the dominant kernel only (every 4th launch): an event pair costs ~10 us of stream time,
    # so the other kernels are timed in a separate, untimed pass
    fused = model._fused()
    dom = "estep_fused" if fused else "scores_gemm"
    chunks_per_step = 1 if fused else max(1, N // model._launch_rows(N))
    if args.full:
        timer = KernelTimer(only={dom}, stride=4 * chunks_per_step)
        model.timer = timer
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last = estep_pass()
    barrier()
    elapsed = time.perf_counter() - t0
    gc.enable()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, data, last)
    del last
    if not args.full:
        mine = torch.tensor([elapsed, float(data_seed), float(N)], dtype=torch.float64, device=dev)
        per_rank = gather_per_rank(mine, world, args.backend, comm)
        elapsed = float(per_rank[:, 0].max())                   # MAX over ranks
        if rank == 0:
            assert len({int(v) for v in per_rank[:, 1]}) == world and all(int(v) == N for v in per_rank[:, 2]), per_rank
            out = headline(args, world, N, elapsed, prewarm_ms)
            out["per_rank"] = [{"rank": r, "ms_per_step": per_rank[r, 0] / args.steps * 1e3, "data_seed": int(per_rank[r, 1]),
                                "rows": int(per_rank[r, 2])} for r in range(world)]
            print(json.dumps(out))
        if world > 1:
            dist.destroy_process_group()
        return
    kern = timer.summary()
    model.timer = all_timer = KernelTimer()
    for _ in range(3):
        estep_pass()
    model.timer = None
    all_kern = all_timer.summary()

    # ---- full EM iterations (select + E + M incl. all-reduce and solve)
    p = dict(params)
    for _ in range(3):
        p = model.step(anneal, p, data)
    gc.collect()
    gc.disable()
    barrier()
    t1 = time.perf_counter()
    em_ts = []
    for _ in range(args.em_steps):
        t2 = time.perf_counter()
        p = model.step(anneal, p, data)
        em_ts.append(time.perf_counter() - t2)
    barrier()
    em_elapsed = time.perf_counter() - t1
    gc.enable()
    if os.environ.get("PM_BENCH_DEBUG"):
        print("em step times ms:", " ".join("%.1f" % (x * 1e3) for x in em_ts), file=sys.stderr)
    # ... and the same loop in its steady state (`em_iter_steady_ms`).  The window above starts three steps after a cold start
    # (first-use allocations, the cold inverse: 36 / 6 / 5 ms steps with an idle GPU in between) and its first ~10 steps run
    # 2.7 -> 2.3 ms although the parameters have stopped moving after the second step (sigma and the mean list length are
    # constant from there; no list overflows): it is `estep_fused` itself that takes 2.04 -> 1.71 ms at constant work -- the
    # clock ramping back up under the MFMA load (scratch/bsc_em_early.py, round 5; scratch/ns_resid.py: the inverse's warm
    # start is accepted from the third step on, that is not it).  150 further steps (~0.35 s) later the loop runs the way a
    # long EM run spends nearly all of its time
    gc.collect()
    gc.disable()
    for _ in range(150):            # (a fixed count: every rank must walk the same sequence of collectives)
        p = model.step(anneal, p, data)
    barrier()
    t1 = time.perf_counter()
    for _ in range(args.em_steps):
        p = model.step(anneal, p, data)
    barrier()
    em_steady = time.perf_counter() - t1
    gc.enable()
    model.timer = em_timer = KernelTimer()
    for _ in range(2):
        model.step(anneal, dict(p), data)
    model.timer = None
    em_kern = em_timer.summary()
    # ... and the reference's own schedule (T and Ncut_factor ramps: the regime 49 of a canonical run's 50 steps are in)
    gc.collect()
    gc.disable()
    annealed = annealed_em(model, params, data, barrier=barrier)
    gc.enable()

    parity = parity_report(BSC_ET, Anneal) if (rank == 0 and cpu is not None) else None
    others = None
    if rank == 0 and world == 1 and not args.no_other_models:
        del Y
        data.clear()
        model.invalidate_data()
        torch.cuda.empty_cache()
        others = other_models(dev, Anneal)
    shapes = None
    if rank == 0 and world == 1 and not args.no_other_shapes:
        if others is None:
            del Y
            data.clear()
            model.invalidate_data()
            torch.cuda.empty_cache()
        shapes = other_shapes(dev, Anneal)

    # the all-reduce of the M-step statistics, timed with events around the collective (EM loop above)
    ar = comm.collective_times()
    allreduce_us = 1e3 * sum(ar) / len(ar) if ar else 0.0
    # per-rank record: what every rank generated and measured (a SCALE record stays attributable)
    mine = torch.tensor([elapsed, em_elapsed, allreduce_us, float(data_seed), float(N), em_steady], dtype=torch.float64,
                        device=dev)
    per_rank = gather_per_rank(mine, world, args.backend, comm)
    elapsed, em_elapsed = float(per_rank[:, 0].max()), float(per_rank[:, 1].max())   # MAX over ranks
    em_steady = float(per_rank[:, 5].max())

    if rank == 0:
        # ... and every rank drew its own rows (seeds differ) -- a shard read twice would double-count throughput
        seeds = [int(v) for v in per_rank[:, 3]]
        assert len(set(seeds)) == world and all(int(v) == N for v in per_rank[:, 4]), (seeds, per_rank[:, 4])
        fused = model._fused()
        dom = "estep_fused" if fused else "scores_gemm"
        chunk = model._dominant_rows(N) if fused else model._launch_rows(N)  # datapoints the dominant launch covers
        # HBM-side bytes of the dominant kernel: NOT measured in this run -- from the committed rocprofv3 --pmc passes
        # (profiles/summarize_pmc.py: FETCH_SIZE x2 gfx950 correction + WRITE_SIZE), per launch
        traffic, traffic_source = None, None
        for fn in PMC_TRAFFIC:
            try:
                pmc = json.load(open(os.path.join(ROOT, "profiles", fn)))["kernels"]
                cands = [k for k, v in pmc.items() if k.startswith(dom) and v.get("datapoints_per_launch") == chunk]
                if cands and N == N_PER_GPU:
                    traffic = pmc[cands[0]]["hbm_bytes"]
                    traffic_source = "profiles/%s (separate rocprofv3 --pmc passes of this command, not this run)" % fn
                    break
            except Exception:
                pass
        sparse_traffic = None
        try:
            if N == N_PER_GPU and traffic_source:
                pmc = json.load(open(os.path.join(ROOT, "profiles", traffic_source.split()[0].split("/")[-1])))["kernels"]
                sparse_traffic = next((v["hbm_bytes"] for k, v in pmc.items() if k.startswith("stats_sparse")), None)
        except Exception:
            pass
        ms_step = elapsed / args.steps * 1e3
        value = world * N * args.steps / elapsed
        dom_ms = kern[dom][1]
        flops = 2.0 * chunk * D * H                        # algorithmic flops of one such launch (524 288 / datapoint)
        achieved = flops / (dom_ms * 1e-3) / 1e12
        K_states = 1 + H + model.no_states
        estep_bytes = N * (D * 8 + HP * 4 + K_states * 8)   # 11 512 B/datapoint
        mfma_roof_dps = MFMA_F64_PEAK_TFLOPS * 1e12 / (2.0 * D * H)      # 150 M datapoints/s
        if fused:
            kname = ("bsc_estep_fused8s_kernel (scores GEMM + select_Hprimes + E_step in one kernel; 8-wavefront tiles, whole "
                     "rounds of the shard; the ragged remainder runs in its TAIL launch, timed apart as estep_fused_tail)"
                     if model._tile8_whole_shard() else
                     "bsc_estep_fused_kernel (scores GEMM + select_Hprimes + E_step, one launch per pass)")
            alg_bytes = chunk * (D * 8 + HP * 4 + (K_states + 1) * 8) + H * D * 8
        else:
            kname = "gemm_nt_f64_dma_kernel (scores A = Y.W^T)"
            alg_bytes = chunk * (D + H) * 8 + H * D * 8
        out = headline(args, world, N, elapsed, prewarm_ms)
        out.update({
            "em_iter_ms": em_elapsed / args.em_steps * 1e3,
            "em_iter_steady_ms": em_steady / args.em_steps * 1e3,
            "em_iter_datapoints_per_s": world * N * args.em_steps / em_elapsed,
            "em_iter_annealed_ms": annealed["em_iter_annealed_ms"],
            "em_iter_annealed": annealed,
            "roofline": {"bound": "mfma", "kernel": kname,
                         "achieved": achieved, "peak": MFMA_F64_PEAK_TFLOPS, "unit": "TFLOP/s",
                         "frac": achieved / MFMA_F64_PEAK_TFLOPS, "traffic": traffic, "traffic_source": traffic_source,
                         "traffic_unit": "bytes/launch (algorithmic: %d)" % alg_bytes,
                         "avg_launch_ms": dom_ms, "datapoints_per_launch": chunk,
                         "launches_per_step": chunks_per_step, "launches_timed": kern[dom][0],
                         # the whole pass (Gram matrix + dominant kernel [+ row kernel]) against both roofs
                         "estep_mfma_frac": (value / world) / mfma_roof_dps,
                         "estep_hbm_frac": (estep_bytes / (ms_step * 1e-3) / 1e9) / HBM_PEAK_GBS,
                         # EM-iteration wall-clock (BASELINE's "+ EM-iter wall-clock"), repeated here because a driver record
                         # keeps this sub-dict: flat schedule (20-step window / steady state) and the reference's own
                         # annealing schedule (EM.run over LinearAnnealing(50), T and Ncut_factor ramps)
                         "em_iter_ms": em_elapsed / args.em_steps * 1e3,
                         "em_iter_steady_ms": em_steady / args.em_steps * 1e3,
                         "em_iter_annealed_ms": annealed["em_iter_annealed_ms"],
                         "em_iter_annealed_ramp_ms": annealed["ramp_ms"],
                         "em_iter_annealed_plateau_ms": annealed["plateau_ms"],
                         "other_models_em_ms": ({k: (round(v, 4) if isinstance(v, float) else
                                                     round(v["em_iter_annealed_ms"], 4))
                                                 for k, v in others.items()
                                                 if k.endswith("_em_iter_ms") or k.endswith("_annealed")}
                                                if others else None),
                         "note": "north_star's '>= 80 % of the HBM roofline' cannot be met in float64: the E-step carries "
                                 "524 288 flop per datapoint against 11 512 B (45 flop/B; machine balance 10 flop/B), so the "
                                 "f64 MFMA roof (150 M datapoints/s) binds at 22 % of the HBM roof; estep_mfma_frac is the "
                                 "whole-pass fraction of that roof, frac the dominant kernel's"},
            "kernels_ms": {k: round(v[1], 4) for k, v in sorted(all_kern.items())},
            "em_kernels_ms": {k: round(v[1], 4) for k, v in sorted(em_kern.items())},
            # the M-step's Wp = E[s]^T Y from the non-zero lists of E[s] (pm_bsc_wp_sparse_f64): bound by streaming the
            # data once (N D 8 algorithmic bytes per launch); the dense product it replaces was MFMA-bound at 1.49 ms
            "em_stats_roofline": ({"bound": "hbm", "kernel": "bsc_wp_sparse_kernel (Wp from the non-zero lists of E[s])",
                                   "achieved": N * D * 8 / (em_kern["stats_sparse"][1] * 1e-3) / 1e9, "peak": HBM_PEAK_GBS,
                                   "unit": "GB/s",
                                   "frac": N * D * 8 / (em_kern["stats_sparse"][1] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                   "avg_launch_ms": em_kern["stats_sparse"][1], "traffic": sparse_traffic,
                                   "traffic_source": traffic_source if sparse_traffic else None}
                                  if "stats_sparse" in em_kern else None),
            "per_rank": [{"rank": r, "ms_per_step": per_rank[r, 0] / args.steps * 1e3,
                          "em_iter_ms": per_rank[r, 1] / args.em_steps * 1e3, "allreduce_us": per_rank[r, 2],
                          "data_seed": int(per_rank[r, 3]), "rows": int(per_rank[r, 4])} for r in range(world)],
            "cpu_baseline": cpu,
            "parity": parity,
            "other_models": others,
            "other_shapes": shapes,
        })
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
