"""Deterministic build: every accumulator is quantised with its own category's quantum and stays inside the bound the host
installed -- checked after the fact on the raw statistics of ONE EM step per case (tests/det_audit.py says why that proves
order independence without waiting for a race).

Each case is one `model.step()` on libprosper_hip_det.so (select_Hprimes -> E_step -> M_step; `step`, because the E-step passes
that carry the M-step's statistics run only inside it), recorded by det_audit.audit; the raw buffer is the first argument of the
model's `_finalize` (the all-reduced packed statistics, before the solve touches them), copied at that moment.  The reference is
the oracle's statistics of the same step (`log["stats"]` of oracle/*_oracle.py); the sums whose addends change sign -- Wp, the
data sums, the sum of log-evidences -- are formed again in np.longdouble from the oracle's per-datapoint posteriors, the
same-sign ones are taken as the oracle's f64 sums (their error, N 2^-53 relative, is far below the tolerance's 1e-9 term).

Routing, asserted from the recorded calls.  Two rows differ from the plan this module was written to:
  * bsc_fused8 runs with `model.defer_stats = False`: in the deterministic build the 8-wavefront pass otherwise takes the deferred
    form on EVERY step (BSC_ET._want_ms), so pm_bsc_estep_fused8_nz_f64 -- and the PM_Q sites of its accumulating epilogue --
    would never run; bsc_fused8_cut keeps the default and covers the deferred records + pm_bsc_defer_apply_f64.
  * gsc, gsc_g5 audit the FIRST step of a loop (host bounds, pm_gsc_estep_f64 + the dense contraction): from the second step on
    the quanta come from a kernel (pm_gsc_det_quanta_f64) that no host-side shift reaches -- the list pass, the gathered GEMM
    and the transposed sparse product are audited at their real quanta in test_gsc_list_pass_at_the_device_quanta.

PM_Q site (file:line) -> case that covers it
  bsc_kernels.hip:257,276,279,287,306              bsc_wave64 (pm_bsc_mstep_rows_f64)
  bsc_rows16.hip:259,265,326,327,345               bsc_rows16 (pm_bsc_mstep_rows16[_nz]_f64), bsc_mu
  bsc_rows16_body.h:656,669; bsc_fused.hip:297     bsc_fused (pm_bsc_estep_fused_f64 with statistics); the body is also compiled
                                                   into bsc_rows16.hip (bsc_rows16) and bsc_fused8.hip (bsc_fused8)
  bsc_fused8.hip:857,879,884,908,970               bsc_fused8, bsc_dense_wp (pm_bsc_estep_fused8_nz_f64)
  bsc_fused8.hip:1041,1064,1068,1085               bsc_fused8_cut (pm_bsc_defer_apply_f64)
  bsc_wp_sparse.hip:146,173                        bsc_fused8, bsc_fused8_cut, bsc_rows16 (pm_bsc_wp_sparse[_expand]_f64)
  gemm_f64.hip:506,666                             bsc_wave64, bsc_fused, bsc_dense_wp, mca, dsc (pm_gemm_tn_acc[_gated]_f64)
  gemm_f64.hip:721                                 test_column_reductions (pm_col_moments_f64)
  gemm_f64.hip:741                                 bsc_mu, test_column_reductions (pm_col_sum_kept_f64)
  gemm_f64.hip:389                                 none: pm_gemm_nt_f64's K-slices, which the deterministic build never takes
  mca_kernels.hip:784,850,851,877                  mca, mmca (pm_mca_estep_mstats_defer_f64 accumulating; mmca: signed instantiation)
  mca_kernels.hip:987,1123,1124,1149               mca_rows (pm_mca_mstep_rows_f64: a truncation step with defer_stats = False)
  mca_kernels.hip:1430,1456,1537,1538,1541,1542    mca_cut (pm_mca_defer_apply_f64)
  dsc_kernels.hip:693,744,756,757,762              dsc_rows16, tsc (pm_dsc_estep_mstats_f64; tsc: the table-only flag)
  dsc_kernels.hip:863,908,919,920,924              dsc_wave64 (pm_dsc_mstep_rows_f64 where the sixteen-lane layout does not fit: H = 300)
  dsc_kernels.hip:1044,1126,1138,1139,1144         dsc (fuse_mstats = False: pm_dsc_mstep_rows_nz_f64), dsc_rows16_cut (..._cutp_f64)
  gsc_kernels.hip:288,290,677,687,738,739          gsc, gsc_g5 (pm_gsc_estep_f64), test_gsc_list_pass_at_the_device_quanta (..._lists_f64)
"""
import ctypes
import functools

import numpy as np
import pytest

import det_audit as A

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

UP = {c: 12 + 4 * c for c in range(5)}
DOWN = {c: 12 + 4 * (4 - c) for c in range(5)}
SCALES = ("y", "1e3", "1e-3", "+50", "col100")


class _An(dict):
    crit_params = []

    def __missing__(self, k):
        return 0.0

    def as_dict(self):
        return dict(self)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU box (MI355X)")
    return torch.device("cuda", 0)


# --------------------------------------------------------------------------------------------------------------- the cases
# family, (D, H, H', gamma, N), annealing point, options, entry points that must have run (prefix match; a tuple = any of them)
_SHARP = dict(strong=1.5, weak=6, wnoise=0.1, sigma=1.0)       # see _column_scales
_CASES = {
    "bsc_wave64": ("bsc", (20, 12, 5, 3, 700), dict(T=2.0), dict(attrs=dict(use_rows16=False)),
                   ["pm_bsc_mstep_rows_f64", "pm_gemm_tn_acc_f64"]),
    "bsc_rows16": ("bsc", (64, 300, 8, 5, 1000), dict(T=1.0), dict(pi=2.5 / 300, **_SHARP), ["pm_bsc_mstep_rows16"]),
    "bsc_fused": ("bsc", (40, 30, 8, 5, 900), dict(T=2.0), dict(), ["pm_bsc_estep_fused_f64"]),
    "bsc_fused8": ("bsc", (64, 160, 8, 3, 1500), dict(T=1.0), dict(attrs=dict(defer_stats=False), pi=2.5 / 160, **_SHARP),
                   ["pm_bsc_estep_fused8_nz_f64", "pm_bsc_wp_sparse"]),
    "bsc_fused8_cut": ("bsc", (64, 160, 8, 3, 1500), dict(T=1.0, Ncut_factor=0.6), dict(pi=2.5 / 160, **_SHARP),
                       ["pm_bsc_estep_fused8_defer_f64", "pm_bsc_defer_apply_f64", "pm_bsc_wp_sparse"]),
    "bsc_dense_wp": ("bsc", (64, 160, 8, 3, 1500), dict(T=60.0), dict(attrs=dict(defer_stats=False), pi=0.6),
                     ["pm_bsc_estep_fused8_nz_f64", "pm_gemm_tn_acc_gated_f64"]),
    "bsc_mu": ("bsc", (20, 12, 5, 3, 700), dict(T=2.0), dict(mu=True), ["pm_col_sum_kept_f64"]),
    "mca": ("mca", (64, 128, 8, 3, 900), dict(T=1.5), dict(), ["pm_mca_estep_mstats_defer_f64", "pm_gemm_tn_acc_f64"]),
    "mca_cut": ("mca", (64, 128, 8, 3, 900), dict(T=1.5, Ncut_factor=0.6), dict(), ["pm_mca_defer_apply_f64"]),
    "mca_rows": ("mca", (64, 128, 8, 3, 900), dict(T=1.5, Ncut_factor=0.6), dict(attrs=dict(defer_stats=False)),
                 ["pm_mca_mstep_rows_f64"]),
    "mmca": ("mmca", (64, 40, 6, 3, 600), dict(T=1.2), dict(), ["pm_mca_estep_mstats_defer_f64"]),
    "dsc": ("dsc", (32, 24, 5, 3, 900), dict(T=1.5), dict(attrs=dict(fuse_mstats=False)),
            ["pm_dsc_mstep_rows_nz_f64", "pm_wp_sparse_f64"]),
    "dsc_wave64": ("dsc", (64, 300, 5, 3, 900), dict(T=1.0), dict(_SHARP, strong=2.0), ["pm_dsc_mstep_rows_f64", "pm_gemm_tn_acc_f64"]),
    "dsc_rows16": ("dsc", (96, 128, 6, 3, 1500), dict(T=1.0), dict(**_SHARP), ["pm_dsc_estep_mstats_f64", "pm_wp_sparse_f64"]),
    "dsc_rows16_cut": ("dsc", (96, 128, 6, 3, 1500), dict(T=1.0, Ncut_factor=0.6), dict(**_SHARP),
                       ["pm_dsc_mstep_rows_cutp_f64", "pm_wp_sparse_f64"]),
    "tsc": ("tsc", (96, 128, 6, 3, 1500), dict(T=1.0), dict(**_SHARP), ["pm_dsc_estep_mstats_f64", "pm_wp_sparse_f64"]),
    # GSC, first step of a loop: the quanta come from the host's bounds (GSC._det_quanta), the plain E-step kernel and the dense
    # contraction run.  (The list pass of later steps takes its quanta from a kernel: test_gsc_list_pass_at_the_device_quanta.)
    "gsc": ("gsc", (128, 128, 6, 3, 1200), dict(T=1.0), dict(strong=0.6, mu=2.5), ["pm_gsc_estep_f64", "pm_gemm_tn_acc_f64"]),
    "gsc_g5": ("gsc", (48, 40, 7, 5, 600), dict(T=1.0), dict(), ["pm_gsc_estep_f64", "pm_gemm_tn_acc_f64"]),
}
_BOUND_CASES = ("bsc_wave64", "bsc_fused8", "bsc_mu", "mca", "mmca", "dsc", "tsc", "gsc")
_DSC_STATES = np.array([-1.0, 0.0, 1.0, 2.0])


def _column_scales(H, opt):
    """Per-latent amplitude of a generating W: `strong` for all but the last `weak` latents, 0.25 for those.  Why: a state more
    than 37 nats below a datapoint's best is not evaluated by the row kernels, so with strong columns the wrong latents drop
    out exactly (sparse E[s] rows, few non-zero pair entries, each a count of real co-activations), while the few weak
    ones keep the posteriors -- and with them the addends -- fractional."""
    s = np.full(H, float(opt.get("strong", 1.0)))
    if opt.get("weak", 0):
        s[H - int(opt["weak"]):] = 0.25
    return s[None, :]


def _rescale(p, y, scale, family):
    """The five data scalings of the bounds test.  sigma moves with the data so the posteriors stay spread."""
    p = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    if scale == "y":
        return p, y
    if family == "gsc":                           # (the latents keep their scale: W, the noise and the data move)
        if scale in ("1e3", "1e-3"):
            f = float(scale)
            p["W"], p["sigma_sq"] = p["W"] * f, p["sigma_sq"] * f * f
            return p, y * f
        if scale == "+50":
            y2 = y + 50.0
            p["sigma_sq"] = p["sigma_sq"] * float((y2 * y2).mean() / (y * y).mean())
            return p, y2
        p["W"][:, 0] *= 100.0
        return p, y
    if scale in ("1e3", "1e-3"):
        f = float(scale)
        p["W"] = p["W"] * f
        p["sigma"] = p["sigma"] * f
        if "mu" in p:
            p["mu"] = p["mu"] * f
        return p, y * f
    if scale == "+50":
        y2 = y + 50.0
        p["sigma"] = p["sigma"] * float(np.sqrt((y2 * y2).mean() / (y * y).mean()))
        return p, y2
    assert scale == "col100"
    p["W"][:, 0] *= 100.0
    return p, y


@functools.lru_cache(maxsize=None)
def _scenario(case, scale="y"):
    """Model factory, parameters, data and annealing point of a case (deterministic in its name)."""
    family, (D, H, Hp, g, N), an, opt, must = _CASES[case]
    rng = np.random.RandomState(sum(map(ord, case)) % 1000)
    extra = {}
    if family == "bsc":
        from oracle import bsc_oracle as O
        from prosper_amd.em.camodels.bsc_et import BSC_ET
        W = rng.normal(size=(D, H)) * _column_scales(H, opt)
        y = O.generate_bsc_data(W, 2.0 / H, 1.0, N, rng)[0]
        p = {"W": W + opt.get("wnoise", 0.3) * rng.normal(size=(D, H)) * _column_scales(H, opt),
             "pi": opt.get("pi", 3.0 / H), "sigma": opt.get("sigma", 1.6)}
        learn = ["W", "pi", "sigma"]
        if opt.get("mu"):
            mu = rng.normal(size=D) * 0.7
            y = y + mu
            p["mu"] = mu + 0.1 * rng.normal(size=D)
            learn = learn + ["mu"]
        make = lambda: BSC_ET(D, H, Hp, g, to_learn=list(learn))
    elif family in ("mca", "mmca"):
        if family == "mca":
            from oracle import mca_oracle as O
            from prosper_amd.em.camodels.mca_et import MCA_ET as cls
            W = np.abs(rng.normal(size=(D, H))) * 3 + 0.1
            y = O.generate_mca_data(W, 2.0 / H, 1.0, N, rng)[0]
        else:
            from oracle import mmca_oracle as O
            from prosper_amd.em.camodels.mmca_et import MMCA_ET as cls
            W = rng.normal(size=(D, H)) * 3.0
            y = O.generate_from_hidden(W, rng.random_sample((N, H)) < 2.0 / H) + rng.normal(size=(N, D))
        p = {"W": W * rng.uniform(0.85, 1.15, size=W.shape), "pi": 3.0 / H, "sigma": 2.5}
        make = lambda: cls(D, H, Hp, g)
    elif family == "dsc":
        from prosper_amd.em.camodels.dsc_et import DSC_ET
        W = rng.normal(size=(D, H)) * _column_scales(H, opt)
        a = min(0.12, 2.5 / H)                                            # about 2.5 active latents per datapoint
        s = _DSC_STATES[rng.choice(4, size=(N, H), p=[a / 3, 1 - a, 5 * a / 12, a / 4])]
        y = s @ W.T + rng.normal(size=(N, D))
        p = {"W": W + opt.get("wnoise", 0.3) * rng.normal(size=(D, H)) * _column_scales(H, opt),
             "pi": np.array([0.06, 0.82, 0.07, 0.05]), "sigma": opt.get("sigma", 1.6)}
        make = lambda: DSC_ET(D, H, Hp, g, states=_DSC_STATES.copy())
    elif family == "gsc":
        from oracle import gsc_oracle as O
        from prosper_amd.em.camodels.gsc_et import GSC
        # (case gsc: slab mean 2.5 on columns of norm^2 0.36 D, found by a scan on the CPU: a pair of latents that is active together
        # ONCE then already puts 64 coarse quanta into its entry of xs^T xsz -- most non-zero entries of the H x H blocks are such pairs)
        gt = {"W": rng.normal(size=(D, H)) * opt.get("strong", 1.0), "pi": np.full(H, 2.0 / H), "mu": np.full(H, opt.get("mu", 1.5)),
              "psi_sq": np.eye(H), "sigma_sq": 1.0}
        y = O.generate_gsc_data(gt, N, rng)[0]
        p = {"W": gt["W"] + 0.1 * rng.normal(size=(D, H)), "pi": gt["pi"] * 1.1, "mu": gt["mu"] + 0.1 * rng.normal(size=H),
             "psi_sq": np.diag(rng.uniform(0.7, 1.4, size=H)), "sigma_sq": 1.2}
        make = lambda: GSC(D, H, Hp, g, "scalar")
    else:
        from prosper_amd.em.camodels.tsc_et import TSC_ET
        W = rng.normal(size=(D, H)) * _column_scales(H, opt)
        s = rng.choice([-1., 0., 1.], size=(N, H), p=[1.0 / H, 1 - 2.0 / H, 1.0 / H])
        y = s @ W.T + rng.normal(size=(N, D))
        p = {"W": W + opt.get("wnoise", 0.3) * rng.normal(size=(D, H)) * _column_scales(H, opt), "pi": 3.0 / H,
             "sigma": opt.get("sigma", 2.0)}
        make = lambda: TSC_ET(D, H, Hp, g)
    p, y = _rescale(p, y, scale, family)
    return dict(family=family, shape=(D, H, Hp, g, N), an=dict(an), attrs=opt.get("attrs", {}), must=must, make=make, p=p, y=y,
                **extra)


def _softmax(lp):
    q = np.exp(lp - lp.max(axis=1, keepdims=True))
    return q / q.sum(axis=1, keepdims=True)


def _lse(lp):
    m = lp.max(axis=1)
    return m + np.log(np.exp(lp - m[:, None]).sum(axis=1))


def _ld(x):
    return np.asarray(x, dtype=np.longdouble)


@functools.lru_cache(maxsize=None)
def _reference(case, scale="y"):
    """The oracle's step -> name -> (reference value, sum of |addend| or None where only the final value bounds it).  Names as
    `_derived` returns them."""
    sc = _scenario(case, scale)
    D, H, Hp, g, N = sc["shape"]
    fam, an, p, y = sc["family"], sc["an"], sc["p"], sc["y"]
    copy = lambda: {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    T, ncut = an.get("T", 1.0), an.get("Ncut_factor", 0.0)
    out = {}
    if fam == "bsc":
        from oracle import bsc_oracle as O
        om = O.make_model(D, H, Hp, g)
        _, log = O.em_step(O.Anneal(T=T, Ncut_factor=ncut, anneal_prior=False), om, copy(), y, stats_fn=O.m_step_stats_vec,
                           vec=True)
        st, keep = log["stats"], log["keep"]
        lp, cand, yk = log["logpj"][keep], log["candidates"][keep], y[keep]
        q = _softmax(lp)
        Es = q[:, 1:H + 1].copy()
        np.add.at(Es, (np.arange(len(yk))[:, None], cand), q[:, H + 1:] @ om["SM"].astype(np.float64))
        lse = _lse(lp)
        out["Wp"] = (_ld(Es).T @ _ld(yk), np.abs(Es).T @ np.abs(yk))             # raw Wp is against y, not y - mu
        out["Wq"] = (st["Wq"], None)
        out["mus"] = (_ld(Es).sum(axis=0), None)
        out["sum_qe"] = (st["sigma"], None)
        out["sum_lse"] = (_ld(lse).sum(), np.abs(lse).sum())
        out["kept"] = (float(log["N_use"]), None)
        if "mu" in p:
            out["data_sum"] = (_ld(yk).sum(axis=0), np.abs(yk).sum(axis=0))
        return out
    if fam in ("mca", "mmca"):
        if fam == "mca":
            from oracle import mca_oracle as O
        else:
            from oracle import mmca_oracle as O
        om = O.make_model(D, H, Hp, g)
        _, log = O.em_step(O.Anneal(T=T, Ncut_factor=ncut), om, copy(), y, vec=True)
        st = log["stats"]
        lpb = log["logpj"] / T
        den = _lse(lpb)
        keep = np.ones(N, dtype=bool)
        if ncut > 0:
            A_pg = O.pi_gamma_factors(p["pi"], H, g)[0]
            keep = den >= np.sort(den, kind="mergesort")[-int(N * (1 - (1 - A_pg) * ncut))]
        assert int(keep.sum()) == log["N_use"]
        q1 = _softmax(lpb[keep])[:, 1:H + 1]
        lse1 = _lse(log["logpj"][keep])
        out["G1"] = (_ld(q1).T @ _ld(y[keep]), np.abs(q1).T @ np.abs(y[keep]))
        out["Wp"] = (st["Wp"], None)
        out["Wq"] = (st["Wq"], None)
        out["q1sum"] = (q1.sum(axis=0), None)
        out["pi"] = (st["pi"], None)
        out["sum_qe"] = (st["sigma"], None)
        out["sum_lse"] = (_ld(lse1).sum(), np.abs(lse1).sum())
        out["kept"] = (float(log["N_use"]), None)
        out["_W"] = (O.check_params(copy())["W"], None)
        return out
    if fam == "gsc":
        from oracle import gsc_oracle as O
        _, log = O.em_step(O.Anneal(T=T), O.make_model(D, H, Hp, g), copy(), y)
        f = log["suff"]
        xs, xsz = f["xpt_s"], f["xpt_sz"]
        out["Wp"] = (_ld(y).T @ _ld(xsz), np.abs(y).T @ np.abs(xsz))
        out["xs_xsz"] = (_ld(xs).T @ _ld(xsz), np.abs(xs).T @ np.abs(xsz))
        out["xsz_xsz"] = (_ld(xsz).T @ _ld(xsz), np.abs(xsz).T @ np.abs(xsz))
        out["sum_ss"] = (f["xpt_ss"].sum(axis=0), None)
        out["sum_zz"] = (_ld(f["xpt_szsz"]).sum(axis=0), np.abs(f["xpt_szsz"]).sum(axis=0))
        out["sum_s"] = (xs.sum(axis=0), None)
        out["sum_sz"] = (_ld(xsz).sum(axis=0), np.abs(xsz).sum(axis=0))
        return out
    if fam == "dsc":
        from oracle import dsc_oracle as O
        om = O.make_model(D, H, Hp, g, _DSC_STATES.copy())
    else:
        from oracle import tsc_oracle as O
        om = O.make_model(D, H, Hp, g)
    _, log = O.em_step(O.Anneal(T=T, Ncut_factor=ncut, anneal_prior=False), om, copy(), y, vec=True)
    st = log["stats"]
    lp = log["logpj"]
    lse = _lse(lp)
    keep = np.ones(N, dtype=bool)
    if ncut > 0:
        A_pg = O.scaling_factor(om, p["pi"]) if fam == "dsc" else O.pi_gamma_factors(p["pi"], H, g)[0]
        with np.errstate(under="ignore"):
            den = np.exp(lp).sum(axis=1)                                  # (un-stabilised, as the reference ranks them)
        cut = np.sort(den, kind="mergesort")[-int(N * (1 - (1 - A_pg) * ncut))]
        keep = (den > cut) if fam == "dsc" else (den >= cut)
    assert int(keep.sum()) == log["N_use"]
    out["Wp"] = (st["Wp"], None)
    out["Wq"] = (st["Wq"], None)
    out["sum_qe"] = (st["sigma"] * (D if fam == "dsc" else 1.0), None)
    out["sum_lse"] = (_ld(lse[keep]).sum(), np.abs(lse[keep]).sum())
    out["kept"] = (float(log["N_use"]), None)
    if fam == "dsc":
        out["counts"] = (st["pi"], None)
        out["_K0"] = (om["K_0"], None)
    return out


# ------------------------------------------------------------------------------------------------------------ one EM step
class _Step(object):
    pass


class _Comm(object):
    """The model's communicator, copying the first buffer of `n` doubles it is asked to all-reduce."""

    def __init__(self, inner, got, n):
        self._inner, self._got, self._n = inner, got, n

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def allreduce_device(self, t, *a, **kw):
        out = self._inner.allreduce_device(t, *a, **kw)
        if t.numel() == self._n and "raw" not in self._got:
            self._got["raw"] = t.detach().cpu().numpy().copy()
        return out


def _run(case, shifts=None, scale="y"):
    """One `step` of the case on the deterministic library under the recorder -> raw statistics, record, block map."""
    from prosper_amd import _lib
    sc = _scenario(case, scale)
    D, H, Hp, g, N = sc["shape"]
    m = sc["make"]()
    m.deterministic = True
    for k, v in sc["attrs"].items():
        setattr(m, k, v)
    np.random.seed(20)              # (GSC's host fallback for a singular sum of xpt_szsz draws its regulariser from np.random, as
    got = {}                        # the reference does: two runs agree only from the same seed)

    def finalize(stats, *a, **kw):
        got["raw"] = stats.detach().cpu().numpy().copy()
        return type(m)._finalize(m, stats, *a, **kw)

    if sc["family"] == "gsc":                   # (GSC has no _finalize: the buffer it hands to the all-reduce)
        m.comm = _Comm(m.comm, got, A.gsc_blocks(H, D)[1]["n"])
    else:
        m._finalize = finalize
    p = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in sc["p"].items()}
    with A.audit(m, shifts) as rec:
        new = m.step(_An(**sc["an"]), p, {"y": sc["y"]})
        torch.cuda.synchronize()
    r = _Step()
    r.raw, r.rec, r.new, r.model, r.sc = got["raw"], rec, new, m, sc
    lib = _lib.load(True)
    if sc["family"] == "bsc":
        r.blocks, r.lay = A.bsc_blocks(H, D, lib, rec, learn_mu="mu" in m.to_learn)
        o_sc = r.lay["o_sc"]
        if r.raw[o_sc + 3] != 0.0:            # a list overflowed: the sparse product returned at once, the dense one did the work
            r.blocks[0] = r.blocks[0]._replace(unit="gemm")
    elif sc["family"] in ("mca", "mmca"):
        r.blocks, r.lay = A.mca_blocks(H, D, lib, rec)
    elif sc["family"] == "gsc":
        r.blocks, r.lay = A.gsc_blocks(H, D)
    else:
        r.blocks, r.lay = A.dsc_blocks(H, D, lib, rec, 8, table_only=sc["family"] == "tsc")
        if r.raw[r.lay["o_sc"] + 3] != 0.0:
            r.blocks[0] = r.blocks[0]._replace(unit="gemm")
        if sc["family"] == "tsc":
            assert not r.raw[_block(r, "qdiag").sl].any(), "TSC: the singleton diagonal is expected to stay unused"
    for want in sc["must"]:
        alts = want if isinstance(want, tuple) else (want,)
        assert any(rec.ran(w) for w in alts), "%s: none of %r ran; calls: %r" % (case, alts, sorted(set(rec.calls)))
    if case == "bsc_fused":                   # ... WITH statistics: the expectation and statistics pointers of the pass
        a = rec.args["pm_bsc_estep_fused_f64"]
        assert a[23] is not None and a[25] is not None, "pm_bsc_estep_fused_f64 ran without the M-step statistics"
    if case == "bsc_dense_wp":
        assert r.raw[r.lay["o_sc"] + 3] != 0.0, "no non-zero list overflowed: the gated dense product did no work"
    if case == "mmca":
        assert float(m.signed_w) == 1.0
    return r


def _block(r, name):
    return next(b for b in r.blocks if b.name == name)


def _derived(r):
    """name -> (value, tolerance parts [(block name, element-wise factor)]) in the terms the oracle's statistics come in."""
    raw, lay, fam = r.raw, r.lay, r.sc["family"]
    D, H = r.sc["shape"][:2]
    v = lambda name: raw[_block(r, name).sl]
    out = {}
    if fam == "gsc":
        shp = {"Wp": (D, H), "xs_xsz": (H, H), "xsz_xsz": (H, H), "sum_ss": (H, H), "sum_zz": (H, H), "sum_s": (H,), "sum_sz": (H,)}
        return {k: (v(k).reshape(s_), [(k, 1.0)]) for k, s_ in shp.items()}
    if fam in ("bsc", "dsc", "tsc"):
        U = v("Wq").reshape(H, H)
        out["Wp"] = (v("Wp").reshape(H, D), [("Wp", 1.0)])
        out["Wq"] = (np.triu(U) + np.triu(U, 1).T + np.diag(v("qdiag")), [("Wq", 1.0), ("qdiag", np.eye(H))])
        for k in ("sum_qe", "sum_lse", "kept"):
            out[k] = (v(k)[0], [(k, 1.0)])
        if fam == "bsc":
            out["mus"] = (v("mus"), [("mus", 1.0)])
            if any(b.name == "data_sum" for b in r.blocks):
                out["data_sum"] = (v("data_sum"), [("data_sum", 1.0)])
        if fam == "dsc":
            out["counts"] = (v("counts"), [("counts", 1.0)])
        return out
    HD = lay["HD"]
    G1, Wpm, Wqm, q1s = v("G1").reshape(H, D), v("Wp_multi").reshape(H, D), v("Wq_multi").reshape(H, D), v("q1sum")
    return {"G1": (G1, [("G1", 1.0)]), "q1sum": (q1s, [("q1sum", 1.0)]), "pi": (v("pi")[0], [("pi", 1.0)]),
            "sum_qe": (v("sum_qe")[0], [("sum_qe", 1.0)]), "sum_lse": (v("sum_lse")[0], [("sum_lse", 1.0)]),
            "kept": (v("kept")[0], [("kept", 1.0)]), "_parts": ((G1, Wpm, Wqm, q1s), [])}


def _mca_totals(r, ref):
    """MCA: Wp = G1 W^2 + Wp_multi, Wq = q1sum W^2 + Wq_multi (MMCA: without the W^2) -- as the oracle's statistics have them."""
    G1, Wpm, Wqm, q1s = _derived(r)["_parts"][0]
    W2 = (ref["_W"][0].T ** 2) if r.sc["family"] == "mca" else np.ones_like(G1)
    return {"Wp": (G1 * W2 + Wpm, [("G1", W2), ("Wp_multi", 1.0)]),
            "Wq": (q1s[:, None] * W2 + Wqm, [("q1sum", W2), ("Wq_multi", 1.0)])}


# ------------------------------------------------------------------------------------------------- (a) + (b): coarse quanta
_ORDERS = {"ascending": UP, "descending": DOWN, "aligned-ascending": A.aligned_shifts(False),
           "aligned-descending": A.aligned_shifts(True)}


@pytest.mark.parametrize("order", sorted(_ORDERS))
@pytest.mark.parametrize("case", sorted(_CASES))
def test_blocks_are_multiples_of_their_own_quantum_and_close(dev, case, order):
    """Bounds scaled by 2^(12 + 4 c) (ascending) and 2^(12 + 4 (4 - c)) (descending): coarse quanta, distinct per category;
    and twice more with the quanta of a unit exactly two bits apart in either order (det_audit.aligned_shifts: the fixed shifts
    cannot put the quantum of a category with a 2^17 times larger bound below its neighbour's).
    (a) 100 % of every mapped block is a multiple of the quantum recorded for ITS (unit, category) -- a slot rounded with a
    finer neighbour's quantum, or not at all, is no multiple (by chance: <= 2^-12 per entry); one rounded with a coarser
    neighbour's shows in the other order -- and the pass is not vacuous (det_audit.check_block).
    (b) |got - ref| <= A N q / 2 + 1e-9 max|ref|: half a quantum per addend, derived, plus the suite's rounding term."""
    r = _run(case, _ORDERS[order])
    N = r.sc["shape"][4]
    K = 1 + r.sc["shape"][1] + r.model.no_states if hasattr(r.model, "no_states") else None
    if r.sc["family"] in ("dsc", "tsc"):
        K = r.model._n_logpj()
    for u, b in r.rec.bounds.items():
        print("%s %s: %s bounds %s -> quanta 2^%s" % (case, order, u, ["%.3g" % x for x in b],
                                                      [int(np.log2(A.quantum(M))) for M in r.rec.magics[u][:len(b)]]))
    bad = A.check_multiples(r.raw, r.blocks, r.rec)
    ref = _reference(case)
    got = _derived(r)
    if r.sc["family"] in ("mca", "mmca"):
        got.update(_mca_totals(r, ref))
    for name, (val, parts) in sorted(got.items()):
        if name.startswith("_"):
            continue
        want = np.asarray(ref[name][0], dtype=np.longdouble)
        if name == "counts":                      # (PM_DSC_MAX_K slots, K in use; entry K0 of the counts is unused on the device)
            assert not val[want.size:].any()
            val, want = np.delete(val[:want.size], int(ref["_K0"][0])), np.delete(want, int(ref["_K0"][0]))
        tol = sum(np.asarray(f, dtype=np.float64) * (A.close_tol(_block(r, bn), r.rec, N, K, 0.0)) for bn, f in parts) \
            + 1e-9 * float(np.abs(want).max())
        err = np.abs(np.asarray(val, dtype=np.longdouble) - want)
        print("%s %s: %s max err %.3e, tolerance %.3e" % (case, order, name, float(err.max()), float(np.max(tol))))
        if not (err <= tol).all():
            bad.append("%s: max |got - ref| = %.3e above A N q / 2 + 1e-9 max|ref| = %.3e"
                       % (name, float(err.max()), float(np.max(tol))))
    assert not bad, "%s (%s shifts):\n  " % (case, order) + "\n  ".join(bad)


# ------------------------------------------------------------------------------- (c): the installed bounds, at real quanta
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("case", _BOUND_CASES)
def test_installed_bounds_hold_on_hostile_scales(dev, case, scale):
    """No shifts.  Every block a multiple of its REAL quantum, every category's sum of |addend| within the bound the host
    installed (`_det_set`'s contract), and a second run of the step leaves the same bits.  sum |addend|: |stat| for the
    same-sign categories; |E[s]|^T |Y|, sum |y| and sum |lse_n| from the oracle's per-datapoint values for the signed ones it is
    one line for; |stat| elsewhere (det_audit's "final" blocks)."""
    r = _run(case, None, scale)
    bad = []
    for b in r.blocks:
        if b.exempt:
            continue
        q = r.rec.q(b.unit, b.cat)
        x = r.raw[b.sl]
        if q is None or not np.isfinite(x).all() or not A.is_multiple(x, q).all():
            bad.append("%s: not all multiples of its quantum %r" % (b.name, q))
    ref = _reference(case, scale)
    head = {}
    for b in r.blocks:
        if b.exempt:
            continue
        sumabs = np.abs(r.raw[b.sl]).max()
        alias = b.name if not b.final else None
        if alias is not None and alias in ref and ref[alias][1] is not None:
            sumabs = max(sumabs, float(np.max(ref[alias][1])))
        bound = r.rec.bound(b.unit, b.cat)
        if sumabs > 0:
            key = "%s/%d" % (b.unit, b.cat)
            head[key] = min(head.get(key, np.inf), bound / sumabs)
        if not sumabs <= bound:
            bad.append("%s: sum |addend| = %.6g exceeds the installed bound %.6g of %s category %d"
                       % (b.name, sumabs, bound, b.unit, b.cat))
    print("HEADROOM %s %s %s" % (case, scale, " ".join("%s=%.3g" % kv for kv in sorted(head.items()))))
    again = _run(case, None, scale)
    if not np.array_equal(r.raw, again.raw):
        bad.append("a second run of the same step differs in %d entries of the raw statistics" % int((r.raw != again.raw).sum()))
    # (GSC's parameters are left out: on y + 50 its sum of xpt_szsz is singular and the host fallback regularises it with a draw
    # from np.random, as the reference does -- the statistics above are what the mode promises)
    for k in (r.new if r.sc["family"] != "gsc" else ()):
        if isinstance(r.new[k], np.ndarray) and not np.array_equal(r.new[k], again.new[k]):
            bad.append("a second run of the same step differs in parameter %s (max %.3e; host-inverse fallbacks: %r)"
                       % (k, float(np.nanmax(np.abs(r.new[k] - again.new[k]))), getattr(r.model, "inverse_fallbacks", None)))
    assert not bad, "%s at scale %s:\n  " % (case, scale) + "\n  ".join(bad)


# ---------------------------------------------------------------------------------------- (d): the column reductions' ABI
@pytest.mark.parametrize("N,D", [(1000, 37), (4097, 130)])
def test_column_reductions(dev, N, D):
    """pm_col_moments_f64 (sums, and centred second moments) and pm_col_sum_kept_f64 on the deterministic library with a coarse
    quantum for gemm category 1: every sum a multiple of it and within N q / 2 of math.fsum."""
    import math
    from prosper_amd import _lib
    from prosper_amd.em.camodels import _device
    rng = np.random.RandomState(N + D)
    Y = rng.normal(size=(N, D))
    lse = rng.normal(size=N)
    cut = 0.25
    bound = 40.0 * N * 2.0 ** 14              # |y| < 6.4 here, (y - c)^2 < 40: no partial sum exceeds it
    magic = A.magic_of(bound)
    q = A.quantum(magic)
    M8 = (ctypes.c_double * 8)(*([0.0, magic] + [0.0] * 6))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _device._DET_QUANTA_SET.pop("gemm", None)
    try:
        _lib.call("pm_det_set_quanta", _lib.DET_UNITS["gemm"], M8, st, det=True)
        Yd, ld = torch.from_numpy(Y).cuda(), torch.from_numpy(lse).cuda()
        center = Y.mean(axis=0)
        cd = torch.from_numpy(center).cuda()
        out = torch.zeros((3, D), dtype=torch.float64, device="cuda")
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        _lib.call("pm_col_moments_f64", p(Yd), D, N, D, None, p(out[0]), st, det=True)
        _lib.call("pm_col_moments_f64", p(Yd), D, N, D, p(cd), p(out[1]), st, det=True)
        _lib.call("pm_col_sum_kept_f64", p(Yd), D, N, D, p(ld), ctypes.c_double(cut), p(out[2]), st, det=True)
        torch.cuda.synchronize()
    finally:
        _device._DET_QUANTA_SET.pop("gemm", None)
    got = out.cpu().numpy()
    keep = lse >= cut
    want = [[math.fsum(Y[:, d]) for d in range(D)], [math.fsum((Y[:, d] - center[d]) ** 2) for d in range(D)],
            [math.fsum(Y[keep, d]) for d in range(D)]]
    for name, g_, w_ in zip(("sum", "centred", "kept"), got, np.array(want)):
        assert A.check_block(name, g_, q) == [], A.check_block(name, g_, q)
        assert np.abs(g_ - w_).max() <= N * q / 2, (name, np.abs(g_ - w_).max(), N * q / 2)


# --------------------------------------------------------------- GSC inside an EM loop: quanta derived on the device
def _gsc_loop(steps=6):
    """`steps` EM steps of case gsc on the deterministic library -> per step: the all-reduced buffer, the entry points enqueued,
    and -- where the step consumed a pass the previous M-step had launched -- the sixteen magic constants
    pm_gsc_det_quanta_f64 installed for it (else None)."""
    sc = _scenario("gsc")
    D, H = sc["shape"][:2]
    m = sc["make"]()
    m.deterministic = True
    n = A.gsc_blocks(H, D)[1]["n"]
    bufs, made, calls, quanta = [], [], [], []

    class Comm(_Comm):
        def allreduce_device(self, t, *a, **kw):
            out = self._inner.allreduce_device(t, *a, **kw)
            if t.numel() == n:
                bufs.append(t.detach().cpu().numpy().copy())
            return out

    m.comm = Comm(m.comm, None, n)

    def dev_quanta(*a, **kw):
        rec = type(m)._det_dev_quanta(m, *a, **kw)
        made.append(rec)
        return rec

    m._det_dev_quanta = dev_quanta
    p = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in sc["p"].items()}
    with A.audit(m) as rec:
        for it in range(steps):
            hits, last = m.spec_hits, (made[-1] if made else None)
            p = m.step(_An(T=1.0), p, {"y": sc["y"]})
            torch.cuda.synchronize()
            calls.append(list(rec.calls))
            del rec.calls[:]
            quanta.append(last["q"].cpu().numpy().copy() if (m.spec_hits > hits and last is not None) else None)
    return bufs, calls, quanta, p


def test_gsc_list_pass_at_the_device_quanta(dev):
    """Inside a loop the M-step launches the next E-step itself: the pass writes lists, and its quanta -- and those of the
    gathered GEMM and the sparse product -- come from pm_gsc_det_quanta_f64, which no host-side shift reaches.  At those REAL
    quanta, for every step that consumed such a pass: the three entry points ran, every block is a multiple of the quantum of
    its category, no entry exceeds the power of two the quantum was derived from (2^51 q: below it every addition is exact);
    and a second loop leaves the same bits at every step."""
    D, H = _scenario("gsc")["shape"][:2]
    bufs, calls, quanta, p = _gsc_loop()
    adopted = [it for it, q in enumerate(quanta) if q is not None]
    assert len(bufs) == len(quanta) and len(adopted) >= 2, "steps that consumed a speculated pass: %r" % (adopted,)
    blocks, _ = A.gsc_blocks(H, D)
    bad = []
    for it in adopted:
        ran = calls[it - 1] + calls[it]                  # (the pass itself was enqueued by the previous step's M-step)
        for want in ("pm_gsc_estep_lists_f64", "pm_gemm_tn_acc_rows_f64", "pm_wp_sparse_t_f64"):
            assert want in ran, "step %d: %s did not run (%r)" % (it, want, sorted(set(ran)))
        rec = A.Record()
        rec.magics = {"gsc": tuple(quanta[it][:8]), "gemm": tuple(quanta[it][8:])}
        for b in blocks:
            if b.exempt:
                continue
            q = rec.q(b.unit, b.cat)
            x = bufs[it][b.sl]
            if q is None or not A.is_multiple(x, q).all():
                bad.append("step %d, %s: not all multiples of its quantum %r" % (it, b.name, q))
            elif not np.abs(x).max() <= q * 2.0 ** 51:
                bad.append("step %d, %s: max |stat| %.6g above the bound 2^51 q = %.6g" % (it, b.name, np.abs(x).max(), q * 2.0 ** 51))
            else:
                print("HEADROOM gsc-lists step %d %s/%d %s = %.3g" % (it, b.unit, b.cat, b.name, q * 2.0 ** 51 / np.abs(x).max()))
    bufs2 = _gsc_loop()[0]
    for it in range(len(bufs)):
        if not np.array_equal(bufs[it], bufs2[it]):
            bad.append("step %d: a second loop differs in %d entries of the statistics" % (it, int((bufs[it] != bufs2[it]).sum())))
    assert not bad, "\n  ".join(bad)
