#!/usr/bin/env python3
"""The reference's bars test (examples/barstests/bars-learning.py + param-bars-*.py) on the MI355X path.

    python examples/bars_learning.py [bsc|mca|mmca|dsc|tsc|gsc|mog|mop] [--steps 50] [--N 2000] [--h5]
    python examples/bars_learning.py mog|mop --init kmeans++ [--seed 1]               (both inits side by side)
    python examples/bars_learning.py bsc|mca|mmca --heldout 500 --infer --exact      (MAP states: truncated against exact)

Generates bars data from ground-truth parameters, runs the annealed EM loop through the drop-in classes and
reports how well the learned dictionary matches the bars (mean absolute error after the best permutation).
Under `torchrun --nproc-per-node N` every rank takes its `stride_data` share and the statistics are
all-reduced once per EM step over RCCL.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from prosper_amd.em import EM                                  # noqa: E402
from prosper_amd.em.annealing import LinearAnnealing           # noqa: E402
from prosper_amd.utils import parallel                         # noqa: E402
from prosper_amd.utils.barstest import generate_bars_dict, find_permutation   # noqa: E402
from prosper_amd.utils.datalog import dlog, StoreInMemory      # noqa: E402


def build(name, size, Hprime, gamma, comm):
    """(model, ground-truth parameters) of the bars test of ``name`` at the truncation Hprime / gamma."""
    H, D = 2 * size, size ** 2
    bars = 10 * generate_bars_dict(H)
    if name == "bsc":
        from prosper_amd.em.camodels.bsc_et import BSC_ET as Model
        model = Model(D, H, Hprime, gamma, comm=comm)
        gt = {'W': bars, 'pi': 2. / H, 'sigma': 1.0}
    elif name == "mca":
        from prosper_amd.em.camodels.mca_et import MCA_ET as Model
        model = Model(D, H, Hprime, gamma, comm=comm)
        gt = {'W': bars, 'pi': 2. / H, 'sigma': 1.0}
    elif name == "mmca":
        from prosper_amd.em.camodels.mmca_et import MMCA_ET as Model
        model = Model(D, H, Hprime, gamma, comm=comm)
        gt = {'W': 10 * generate_bars_dict(H, neg_bars=True), 'pi': 2. / H, 'sigma': 1.0}
    elif name == "dsc":
        from prosper_amd.em.camodels.dsc_et import DSC_ET as Model
        model = Model(D, H, Hprime, gamma, states=np.array([-1., 0., 1.]), comm=comm)
        gt = {'W': bars, 'pi': np.array([1. / H, 1 - 2. / H, 1. / H]), 'sigma': 1.0}
    elif name == "tsc":
        from prosper_amd.em.camodels.tsc_et import TSC_ET as Model
        model = Model(D, H, Hprime, gamma, comm=comm)
        gt = {'W': bars, 'pi': 2. / H, 'sigma': 1.0}
    elif name == "mog":     # examples/barstests/param-bars-mog.py of the reference: diagonal covariances
        from prosper_amd.em.mixturemodels.MoG import MoG
        model = MoG(D, H, sigmas_sq_type='diagonal', comm=comm)
        gt = {'W': bars, 'pies': np.ones(H) / H, 'sigmas_sq': np.ones((H, D))}
    elif name == "mop":     # param-bars-mop.py: A = nan (no normalisation)
        from prosper_amd.em.mixturemodels.MoP import MoP
        model = MoP(D, H, comm=comm)
        gt = {'W': bars, 'pies': np.ones(H) / H}
    else:
        from prosper_amd.em.camodels.gsc_et import GSC as Model
        model = Model(D, H, Hprime, gamma, 'scalar', comm=comm)
        gt = {'W': bars / 10., 'pi': np.full(H, 2. / H), 'mu': np.full(H, 5.0), 'psi_sq': np.eye(H),
              'sigma_sq': 1.0}

    return model, gt


def noiseless_mean(name, gt, drawn):
    """The mean of the data given the latents the generator drew (``generate_data`` returns them as ``s``; GSC: ``z``)."""
    W = np.asarray(gt['W'], dtype=np.float64)
    s = np.asarray(drawn['s'])
    if name in ("mog", "mop"):
        return W.T[s.astype(int)]
    if name == "gsc":
        return np.asarray(drawn['z'], dtype=np.float64) @ W.T
    if name in ("mca", "mmca"):      # per dimension the active cause of largest magnitude (MCA: the maximum), 0 without one
        act = np.where(s[:, None, :] != 0, W[None, :, :], 0.0)                  # (N, D, H)
        idx = np.abs(act).argmax(axis=2)
        return np.take_along_axis(act, idx[:, :, None], axis=2)[:, :, 0]
    return s.astype(np.float64) @ W.T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("model", nargs="?", default="bsc", choices=["bsc", "mca", "mmca", "dsc", "tsc", "gsc", "mog",
                                                                      "mop"])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--N", type=int, default=2000)
    ap.add_argument("--size", type=int, default=5)
    ap.add_argument("--h5", action="store_true", help="store every parameter and the objective per EM step in "
                    "output/<script>.<date>/result.h5, as the reference's bars-learning.py does")
    ap.add_argument("--heldout", type=int, default=0, metavar="N",
                    help="also draw N held-out datapoints from the ground truth and print their log-likelihood per "
                    "datapoint under the learned parameters and under the ground-truth ones (DESIGN 4.12)")
    ap.add_argument("--exact", action="store_true",
                    help="with --heldout: also the exact held-out log-likelihood of the learned parameters, summed over "
                    "every latent state (DESIGN 4.13), next to the truncated bound and their difference per datapoint; "
                    "with --reconstruct: also the mean squared error of the exact posterior mean (DESIGN 4.18)")
    ap.add_argument("--reconstruct", action="store_true",
                    help="with --heldout: denoise the held-out datapoints (reconstruct, DESIGN 4.14) and print the mean squared "
                    "error of the noisy data and of the reconstruction against the noiseless data, for the learned and for "
                    "the generating parameters")
    ap.add_argument("--variance", action="store_true",
                    help="with --heldout --reconstruct: also the posterior variance V of every estimate (reconstruct(variance=True), "
                    "DESIGN 4.19) and the calibration ratio sum (yhat - clean)^2 / sum V: 1 in expectation for a model that "
                    "is as sure as it should be, above 1 for an overconfident one")
    ap.add_argument("--samples", type=int, default=0, metavar="M",
                    help="with --heldout --reconstruct: M posterior draws of the noiseless data per datapoint (sample_posterior, "
                    "DESIGN 4.20): the mean squared error of their mean beside the reconstruction's, and the share of clean "
                    "pixels inside the draws' [5 %%, 95 %%] range")
    ap.add_argument("--encode", action="store_true",
                    help="with --heldout: the codes of the held-out datapoints under the learned parameters (encode, DESIGN "
                    "4.23): the mean number of active latents per datapoint, sum_h P(s_h != 0 | y_n), beside the generating "
                    "pi H; with --exact (BSC, MCA, MMCA, the mixtures) also the largest |prob_truncated - prob_exact|")
    ap.add_argument("--infer", action="store_true",
                    help="bsc, mca, mmca with --heldout: the MAP state of every held-out datapoint under the learned parameters "
                    "(inference, H' = 5, gamma = 3) with and without the adaptive re-runs; with --exact (DESIGN 4.26) the share "
                    "of datapoints whose truncated MAP state is the exact one over all 2^H states, for both settings, and "
                    "the mean posterior probability of the exact MAP state")
    ap.add_argument("--exact-em", action="store_true",
                    help="bsc: train the same start parameters twice on the same data and schedule -- truncated (H' = 5, gamma = "
                    "3) and with the posterior over all 2^H states (model.exact = True, DESIGN 4.25) -- and print the bars "
                    "error and log_likelihood(exact=True) per datapoint of both end points side by side")
    ap.add_argument("--init", choices=["standard", "kmeans++"], default="standard",
                    help="mog, mop with kmeans++: train the same data twice on the same schedule -- from standard_init (H "
                    "components at the data mean) and from kmeanspp_init (H datapoints by D^2 sampling on the device, DESIGN "
                    "4.27) -- and print the bars error and log_likelihood per datapoint of both end points, and the seeding "
                    "potential beside the potential of H uniformly drawn rows")
    ap.add_argument("--seed", type=int, default=1, help="seed of NumPy's generator (data, standard_init) and of the seeding")
    a = ap.parse_args()
    if a.init != "standard" and a.model not in ("mog", "mop"):
        ap.error("--init kmeans++ is built for mog and mop")
    if a.exact_em and a.model != "bsc":
        ap.error("--exact-em is built for bsc")
    if a.infer and (a.model not in ("bsc", "mca", "mmca") or a.heldout <= 0):
        ap.error("--infer is built for bsc, mca and mmca and needs --heldout N")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        dist.init_process_group("nccl")
    comm = parallel.Comm()
    np.random.seed(a.seed + comm.rank)

    model, gt = build(a.model, a.size, 5, 3, comm)
    H = 2 * a.size

    first, last = parallel.stride_data(a.N, comm=comm)
    my_data = model.generate_data(gt, last - first)
    init = model.standard_init(my_data)
    heldout = None
    if a.heldout > 0:
        hf, hl = parallel.stride_data(a.heldout, comm=comm)
        drawn = model.generate_data(gt, hl - hf)
        heldout = {'y': drawn['y']}
        clean = noiseless_mean(a.model, gt, drawn)

    def schedule():
        anneal = LinearAnnealing(a.steps)
        anneal['T'] = [(0, 2.), (.7, 1.)]
        anneal['Ncut_factor'] = [(0, 0.), (2. / 3, 1.)]
        anneal['anneal_prior'] = False
        return anneal

    if a.exact_em:
        ends = {}
        for exact in (False, True):
            model.exact = exact
            start = {k: np.array(v, copy=True) if np.ndim(v) else v for k, v in init.items()}
            em = EM(model=model, anneal=schedule(), data={'y': my_data['y']}, lparams=start)
            em.run()
            model.exact = False
            _, mae = find_permutation(np.asarray(em.lparams['W']), np.asarray(gt['W']))
            ll = model.log_likelihood(dict(em.lparams), {'y': my_data['y']}, exact=True) / a.N
            ends[exact] = (mae, ll, float(em.lparams['pi']), float(em.lparams['sigma']))
        if comm.rank == 0:
            print("BSC on %d bars datapoints (%d ranks), %d EM steps from the same start, H = %d:" % (a.N, comm.size, a.steps, H))
            print("  %-28s %14s %14s" % ("", "truncated 5/3", "exact 2^H"))
            for i, what in enumerate(("bars mean abs error", "exact log-likelihood / N", "pi", "sigma")):
                print("  %-28s %14.6f %14.6f" % (what, ends[False][i], ends[True][i]))
        return

    if a.init == "kmeans++":
        seeded = model.kmeanspp_init(my_data, seed=a.seed)
        all_y = np.concatenate(comm.allgather(np.asarray(my_data['y'], dtype=np.float64)))
        rows = all_y[np.random.RandomState(a.seed).choice(len(all_y), size=H, replace=False)]
        uniform = float(((all_y[:, None, :] - rows[None, :, :]) ** 2).sum(2).min(1).sum())
        ends = {}
        for what, start in (("standard", init), ("kmeans++", seeded)):
            start = {k: np.array(v, copy=True) for k, v in start.items()}
            em = EM(model=model, anneal=schedule(), data={'y': my_data['y']}, lparams=start)
            em.run()
            _, mae = find_permutation(np.asarray(em.lparams['W']), np.asarray(gt['W']))
            ends[what] = (mae, model.log_likelihood(dict(em.lparams), {'y': my_data['y']}) / a.N)
        if comm.rank == 0:
            print("%s on %d bars datapoints (%d ranks), %d EM steps, seed %d, H = %d:" % (a.model.upper(), a.N, comm.size,
                                                                                       a.steps, a.seed, H))
            print("  %-28s %14s %14s" % ("", "standard_init", "kmeanspp_init"))
            for i, what in enumerate(("bars mean abs error", "log-likelihood / N")):
                print("  %-28s %14.6f %14.6f" % (what, ends["standard"][i], ends["kmeans++"][i]))
            print("  seeding potential %.6g (D^2 sampling) against %.6g (H uniformly drawn rows)" % (
                float(model.seed_potential[-1]), uniform))
        return

    anneal = schedule()
    log = dlog.set_handler(('L', 'Q'), StoreInMemory)
    store = None
    if a.h5:
        from prosper_amd.utils import create_output_path
        from prosper_amd.utils.datalog import StoreToH5
        out_dir = create_output_path("bars_learning_" + a.model, comm=comm)
        store = dlog.set_handler(('W', 'pi', 'sigma', 'sigma_sq', 'mu', 'psi_sq', 'pies', 'sigmas_sq', 'L', 'Q', 'N_use', 'T'),
                                 StoreToH5, out_dir + "result.h5")
    em = EM(model=model, anneal=anneal, data={'y': my_data['y']}, lparams=init)
    em.run()
    if store is not None:
        store.close()
        if comm.rank == 0:
            print("parameters of every EM step in %sresult.h5" % out_dir)
    W = np.asarray(em.lparams['W'])
    W_gt = np.asarray(gt['W'])
    if a.model == "gsc":      # the scale of a column trades against the scale of its latent: compare shapes
        W, W_gt = W / np.abs(W).max(axis=0, keepdims=True) * 10, W_gt / np.abs(W_gt).max(axis=0, keepdims=True) * 10
    _, mae = find_permutation(np.abs(W) if a.model in ("mmca", "dsc", "tsc", "gsc") else W, np.abs(W_gt))
    if comm.rank == 0:
        trace = log.tables.get('L', log.tables.get('Q', [])) if log is not None else []
        print("%s on %d bars datapoints (%d ranks), %d EM steps: bars recovered with mean abs error %.3f%s" % (
            a.model.upper(), a.N, comm.size, a.steps, mae,
            "; objective %.3f -> %.3f" % (float(trace[0]), float(trace[-1])) if len(trace) else ""))
    if heldout is not None:
        learned = model.log_likelihood(dict(em.lparams), heldout) / a.heldout      # (collective: every rank calls it)
        truth = model.log_likelihood(dict(gt), heldout) / a.heldout
        if comm.rank == 0:
            print("held-out log-likelihood per datapoint (%d datapoints): learned %.4f, ground truth %.4f"
                  % (a.heldout, learned, truth))
        if a.exact:
            exact = model.log_likelihood(dict(em.lparams), heldout, exact=True) / a.heldout
            if comm.rank == 0:
                print("held-out log-likelihood per datapoint of the learned parameters: truncated bound %.6f, exact %.6f, "
                      "difference %.3e" % (learned, exact, exact - learned))
        if a.encode:
            # which causes each held-out datapoint contains: the posterior activation probabilities over the wider truncated
            # state set --reconstruct uses (H' = 7, gamma = 5), summed over the latents -- the generator activates pi H of them
            emodel = model if a.model in ("mog", "mop") else build(a.model, a.size, min(H, 7), min(H, 5), comm)[0]
            _, prob = emodel.encode(dict(em.lparams), heldout)
            if a.model in ("mog", "mop"):
                active = 1.0
            elif a.model == "dsc":
                active = float(H * (1.0 - np.asarray(gt['pi'])[1]))
            else:
                active = float(np.broadcast_to(np.asarray(gt['pi'], dtype=np.float64), (H,)).sum())
            tot = comm.allreduce(np.array([float(prob.sum()), float(prob.shape[0])]))
            if comm.rank == 0:
                print("held-out codes (%d datapoints): mean number of active latents sum_h P(s_h != 0 | y) %.4f, generating "
                      "pi H %.4f" % (a.heldout, tot[0] / tot[1], active))
            if a.exact and a.model in ("bsc", "mca", "mmca", "mog", "mop"):
                _, exact_prob = emodel.encode(dict(em.lparams), heldout, exact=True)
                worst = max(comm.allgather(float(np.abs(prob - exact_prob).max()) if prob.size else 0.0))
                if comm.rank == 0:
                    print("held-out codes: largest |prob_truncated - prob_exact| %.3e" % worst)
        if a.infer:
            # how often the truncated MAP state is the true one: the selection function proposes H' latents, the adaptive loop
            # re-runs only the datapoints whose MAP state fills gamma -- a MAP latent that was never proposed goes unnoticed
            from prosper_amd.em.camodels._device import LoglikPoint
            maps = {ad: model.inference(LoglikPoint(), dict(em.lparams), heldout, topK=1, adaptive=ad)['s'][:, 0]
                    for ad in (True, False)}
            moved = comm.allreduce(np.array([float((maps[True] != maps[False]).any(axis=1).sum())]))[0]
            if comm.rank == 0:
                print("held-out MAP states (%d datapoints, H' = %d, gamma = %d): the adaptive re-runs change %.4f of them"
                      % (a.heldout, model.Hprime, model.gamma, moved / a.heldout))
            if a.exact:
                ex = model.inference(LoglikPoint(), dict(em.lparams), heldout, topK=1, logprob=True, exact=True)
                hit = [float((maps[ad] == ex['s'][:, 0]).all(axis=1).sum()) for ad in (True, False)]
                tot = comm.allreduce(np.array(hit + [float(np.exp(ex['p'][:, 0]).sum())]))
                if comm.rank == 0:
                    print("held-out MAP states: the truncated MAP state is the exact one (all 2^%d states) for %.4f of the "
                          "datapoints with adaptive=True, %.4f with adaptive=False; mean posterior probability of the exact MAP "
                          "state %.4f" % (H, tot[0] / a.heldout, tot[1] / a.heldout, tot[2] / a.heldout))
        if a.reconstruct:
            y = np.asarray(heldout['y'], dtype=np.float64)
            sq = lambda x: float(((np.asarray(x) - clean) ** 2).sum())
            # the posterior mean over a wider truncated state set than training uses (H' = 7, gamma = 5, the reference's
            # settings for inference on the bars): a datapoint with more than gamma bars has no state near it otherwise,
            # and one missed bar of height 10 costs more than the noise of the whole datapoint
            rmodel = model if a.model in ("mog", "mop") else build(a.model, a.size, min(H, 7), min(H, 5), comm)[0]
            sums = comm.allreduce(np.array([sq(y), sq(rmodel.reconstruct(dict(em.lparams), heldout)),
                                            sq(rmodel.reconstruct(dict(gt), heldout)), float(y.size)]))
            if comm.rank == 0:
                print("held-out mean squared error against the noiseless data (%d datapoints): noisy data %.4f, reconstruction "
                      "with the learned parameters %.4f, with the generating parameters %.4f"
                      % (a.heldout, sums[0] / sums[3], sums[1] / sums[3], sums[2] / sums[3]))
            if a.variance:
                # how sure the model is of these estimates: the summed posterior variance against the summed squared error
                cal = []
                for params in (em.lparams, gt):
                    yh, V = rmodel.reconstruct(dict(params), heldout, variance=True)
                    cal += [sq(yh), float(np.asarray(V).sum())]
                cal = comm.allreduce(np.array(cal))
                if comm.rank == 0:
                    print("held-out calibration sum (yhat - clean)^2 / sum V: learned parameters %.4f, generating parameters %.4f "
                          "(mean posterior variance %.4f and %.4f)"
                          % (cal[0] / cal[1], cal[2] / cal[3], cal[1] / sums[3], cal[3] / sums[3]))
            if a.samples > 0:
                # posterior draws of the noiseless data: their mean tends to the reconstruction, and the range
                # between their 5 % and 95 % quantiles should hold about nine clean pixels in ten
                Ys = rmodel.sample_posterior(dict(em.lparams), heldout, n_samples=a.samples, seed=1 + comm.rank)
                lo, hi = np.quantile(Ys, 0.05, axis=0), np.quantile(Ys, 0.95, axis=0)
                dr = comm.allreduce(np.array([sq(Ys.mean(axis=0)), float(((clean >= lo) & (clean <= hi)).sum())]))
                if comm.rank == 0:
                    print("held-out mean squared error of the mean of %d posterior draws %.4f (reconstruction %.4f); share of "
                          "clean pixels inside the draws' [5 %%, 95 %%] range %.4f"
                          % (a.samples, dr[0] / sums[3], sums[1] / sums[3], dr[1] / sums[3]))
            if a.exact:
                # the quantity the truncated reconstruction approximates: the posterior mean over EVERY state;
                # with the generating parameters it is the minimum-mean-square estimate of the noiseless data
                ex = comm.allreduce(np.array([sq(rmodel.reconstruct(dict(em.lparams), heldout, exact=True)),
                                              sq(rmodel.reconstruct(dict(gt), heldout, exact=True))]))
                if comm.rank == 0:
                    print("held-out mean squared error with the learned parameters: noisy data %.4f, truncated reconstruction "
                          "%.4f, exact reconstruction %.4f (generating parameters: truncated %.4f, exact %.4f)"
                          % (sums[0] / sums[3], sums[1] / sums[3], ex[0] / sums[3], sums[2] / sums[3], ex[1] / sums[3]))


if __name__ == "__main__":
    main()
