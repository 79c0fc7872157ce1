"""Equal-error-rate evaluation: the caller on the output side of the hot path.

Mirrors ``embedding_model_GE2E/s5_eval_model.py:16-100`` (``calculate_ERR``): per test batch the
encoder's embeddings -> get_centroids -> get_cos_sim -> sim = w cos + b with w = 1, b = 0 (s5:27-28,
44-46), then a sweep over the 50 thresholds 0.5 + 0.01 i (s5:57) that keeps the threshold where
|FAR - FRR| is smallest.  The cosines and the per-threshold counts run in libge2e_hip.so
(``ge2e_cos_sim``, ``ge2e_eer_counts``); only 100 integers per batch come back to the host, where
the reference's own scalar arithmetic is repeated verbatim -- including its denominators
(s5:81: (N-1)/M/N for FAR, s5:88: M/N for FRR), which are NOT the population sizes the comments
describe, so FAR/FRR are not ratios in [0,1]; a drop-in has to reproduce them, not repair them.
``normalized=True`` gives the textbook rates instead.
"""
from __future__ import annotations

import torch

from . import functional as GF

THRESHOLDS = [0.01 * i + 0.5 for i in range(50)]  # s5:57


def eer_from_counts(counts, N: int, M: int, thresholds=THRESHOLDS, normalized: bool = False):
    """The scalar part of s5:50-98 for one batch.  counts: (T,2) integers [false accepts, own accepts]."""
    diff, EER, EER_thres, EER_FAR, EER_FRR = 1, 0, 0, 0, 0  # s5:50-54
    for thres, (fa, ta) in zip(thresholds, counts):
        fa, ta = int(fa), int(ta)
        if normalized:
            FAR = fa / ((N - 1) * M * N)
            FRR = (N * M - ta) / (N * M)
        else:
            FAR = fa / ((N - 1) / M / N)      # s5:81-83
            FRR = (N * M - ta) / (M / N)      # s5:88-90: sum_i (M - accepted_i)
        if diff > abs(FAR - FRR):             # s5:93-98
            diff = abs(FAR - FRR)
            EER = (FAR + FRR) / 2
            EER_thres = thres
            EER_FAR = FAR
            EER_FRR = FRR
    return {"EER": EER, "thres": EER_thres, "FAR": EER_FAR, "FRR": EER_FRR}


def eer_from_sim(sim_matrix: torch.Tensor, thresholds=THRESHOLDS, normalized: bool = False):
    """(N,M,N) -> dict, (B,N,M,N) -> list of dicts.  One kernel, one (T,2)-per-batch readback."""
    counts = GF.eer_counts(sim_matrix, thresholds).cpu().numpy()
    N, M = sim_matrix.shape[-3], sim_matrix.shape[-2]
    if sim_matrix.dim() == 3:
        return eer_from_counts(counts, N, M, thresholds, normalized)
    return [eer_from_counts(c, N, M, thresholds, normalized) for c in counts]


def calculate_ERR(model, hp, N: int = 4, M: int = 16, test_loader=None, verbose: bool = True):
    """s5:16-100, the reference's signature: ``calculate_ERR(model, hp, N, M)`` writes N, M into ``hp.m_ge2e.test_N`` /
    ``test_M`` (s5:17-18) and builds the test loader from ``hp`` (s5:21) -- here ``data.get_train_test_data_loader``'s
    second result: the ``sv_*.npy`` folder ``hp.m_ge2e.tt_data.test_spects_path`` resident in HBM, batches gathered by one
    kernel.  ``test_loader`` (an iterable of (N,M,T,F) mel batches) replaces that default for callers that have their own.
    Prints the reference's result line per batch and returns the results (the reference returns None)."""
    hp.m_ge2e.test_N, hp.m_ge2e.test_M = N, M  # s5:17-18
    if test_loader is None:
        from .data import get_train_test_data_loader
        _, test_loader = get_train_test_data_loader(hp)   # s5:21
    total = N * M
    results = []
    with torch.no_grad():
        for mel in test_loader:
            mel = torch.reshape(mel, (total, mel.size(2), mel.size(3))).to(hp.general.device)  # s5:32-33
            emb = model(mel)                                                                   # s5:36
            emb = torch.reshape(emb, (N, M, emb.size(1)))                                      # s5:39
            cos = GF.cos_sim(emb, eps=hp.general.small_err)                                    # s5:42-43
            sim = 1.0 * cos + 0.0                                                              # s5:44 (w=1, b=0)
            r = eer_from_sim(sim)
            if verbose:
                print("\nEER : %0.2f (thres:%0.2f, FAR:%0.2f, FRR:%0.2f)" % (r["EER"], r["thres"], r["FAR"], r["FRR"]))
            results.append(r)
    return results


# ---- labelled evaluation: any utterance count per speaker, rows in any order (ge2e_cos_sim_labeled) ------------------------

def eer_from_labeled_counts(counts, n_act: int, r_act: int, thresholds=THRESHOLDS):
    """The sweep of `eer_from_counts` (s5:50-98) for a labelled batch of ``r_act`` counting rows over ``n_act`` counting
    speakers, with the textbook rates: FAR = fa / (r_act (n_act - 1)) (0 when n_act < 2), FRR = (r_act - ta) / r_act (0
    when r_act = 0).  The reference's own denominators (s5:81, 88) need an M -- one utterance count for every speaker --
    that a ragged batch does not have, so only the normalised rates exist here; with equal counts this is
    ``eer_from_counts(counts, N, M, normalized=True)``."""
    n_act, r_act = int(n_act), int(r_act)
    diff, EER, EER_thres, EER_FAR, EER_FRR = 1, 0, 0, 0, 0  # s5:50-54
    for thres, (fa, ta) in zip(thresholds, counts):
        fa, ta = int(fa), int(ta)
        FAR = fa / (r_act * (n_act - 1)) if n_act >= 2 and r_act > 0 else 0
        FRR = (r_act - ta) / r_act if r_act > 0 else 0
        if diff > abs(FAR - FRR):             # s5:93-98
            diff = abs(FAR - FRR)
            EER = (FAR + FRR) / 2
            EER_thres = thres
            EER_FAR = FAR
            EER_FRR = FRR
    return {"EER": EER, "thres": EER_thres, "FAR": EER_FAR, "FRR": EER_FRR}


def evaluate_labeled(model, loader, num_speakers=None, device="cuda:0", thresholds=THRESHOLDS, verbose: bool = True):
    """`calculate_ERR` for a test set as it comes: ``loader`` yields (mel, speaker_ids) with ANY number of utterances per
    speaker, in any order (negative ids: rows to ignore).  Per batch: the embeddings, ONE `cos_sim_labeled(...,
    need_cos=False)` -- the similarity matrix is never materialised -- and one read-back of T * 2 + 2 integers; the dict of
    `eer_from_labeled_counts` with ``n_act`` and ``r_act`` added.  ``num_speakers``: the bound for device ids (host ids are
    compacted per batch)."""
    results = []
    T = len(thresholds)
    with torch.no_grad():
        for mel, speaker_ids in loader:
            emb = model(mel.to(device)).contiguous().float()
            out = GF.cos_sim_labeled(emb, speaker_ids, num_speakers=num_speakers, thresholds=thresholds, need_cos=False)
            back = torch.cat([out.counts.reshape(-1), out.active.reshape(-1)]).cpu().numpy()   # the one read-back
            n_act, r_act = int(back[2 * T]), int(back[2 * T + 1])
            r = eer_from_labeled_counts(back[:2 * T].reshape(T, 2), n_act, r_act, thresholds)
            r["n_act"], r["r_act"] = n_act, r_act
            if verbose:
                print("\nEER : %0.2f (thres:%0.2f, FAR:%0.2f, FRR:%0.2f)" % (r["EER"], r["thres"], r["FAR"], r["FRR"]))
            results.append(r)
    return results


# ---- enrolment and verification: models from one set of utterances, trials from another (ge2e_verify_scores) -------------

class SpeakerBank:
    """A bank of ``num_speakers`` speaker models of dimension ``dim`` on ``device``: the per-speaker sums and counts that
    `functional.enroll_accumulate` fills, and the unit models made from them.  ``enroll`` may be called any number of times;
    ``models()`` finalises lazily and is invalidated by ``enroll``.  Ids are bank indices 0 .. num_speakers - 1; rows with
    any other id are ignored on enrolment."""

    def __init__(self, num_speakers: int, dim: int, device="cuda:0"):
        self.device = torch.device(device)
        self.sums = torch.zeros(int(num_speakers), int(dim), dtype=torch.float32, device=self.device)
        self.cnt = torch.zeros(int(num_speakers), dtype=torch.int32, device=self.device)
        self._models = None
        self._cohort = None          # (cohort bank, n_top, eps_std) of set_cohort
        self._model_stats = None     # the models' (mean, spread) against the cohort: lazily, as _models

    def enroll(self, emb: torch.Tensor, ids) -> None:
        self._models = None
        self._model_stats = None
        GF.enroll_accumulate(self.sums, self.cnt, emb, ids)

    def models(self) -> torch.Tensor:
        if self._models is None:
            self._models = GF.enroll_finalize(self.sums, self.cnt)
        return self._models

    def set_cohort(self, cohort_bank: "SpeakerBank", n_top: int = 300, eps_std: float = 1e-5) -> None:
        """The cohort of impostor speakers that ``normalize=True`` scores against: another bank of the same dimension on
        the same device, a disjoint set of speakers.  The statistics of this bank's models against it are computed on the
        first normalised call and again after every ``enroll`` (of this bank) or ``set_cohort``; the cohort's own models
        are read when they are needed, so the cohort bank may still be enrolled into."""
        if not isinstance(cohort_bank, SpeakerBank):
            raise TypeError("cohort_bank must be a SpeakerBank")
        if cohort_bank.sums.shape[1] != self.sums.shape[1] or cohort_bank.device != self.device:
            raise ValueError(f"the cohort must have dimension {self.sums.shape[1]} on {self.device}")
        if int(n_top) < 1:
            raise ValueError(f"n_top must be at least 1, got {n_top}")
        self._cohort = (cohort_bank, int(n_top), float(eps_std))
        self._model_stats = None

    def _stats(self, rows: torch.Tensor, select, select_min: int) -> torch.Tensor:
        if self._cohort is None:
            raise ValueError("normalize=True needs a cohort: call set_cohort first")
        bank, n_top, eps_std = self._cohort
        return GF.cohort_stats(rows, bank.models(), bank.cnt, n_top=n_top, select=select, select_min=select_min, eps_std=eps_std)

    def model_stats(self) -> torch.Tensor:
        """(num_speakers, 2): mean and spread of every enrolled model's best cohort scores; (0, 1) where nobody is enrolled."""
        if self._cohort is None:
            raise ValueError("normalize=True needs a cohort: call set_cohort first")
        if self._model_stats is None:
            self._model_stats = self._stats(self.models(), self.cnt, 1)
        return self._model_stats

    def score(self, emb: torch.Tensor, normalize: bool = False) -> torch.Tensor:
        """(R, D) -> scores (R, num_speakers): the cosine of every row with every enrolled model (+ eps), 0 elsewhere.
        ``normalize=True``: AS-norm against the cohort of ``set_cohort``."""
        if not normalize:
            return GF.verify_scores(emb, self.models(), self.cnt).scores
        model_stats = self.model_stats()
        return GF.verify_scores_normed(emb, self.models(), self.cnt, self._stats(emb, None, 0), model_stats).scores

    def verify(self, emb: torch.Tensor, ids, thresholds=THRESHOLDS, need_scores: bool = True,
               normalize: bool = False) -> GF.VerifyOutputs:
        """Labelled trials: scores, accept counts per threshold and the numbers of impostor and target trials.
        ``normalize=True``: scores and counts of the AS-normalised scores (``thresholds`` are then on that scale)."""
        if not normalize:
            return GF.verify_scores(emb, self.models(), self.cnt, labels=ids, thresholds=thresholds, need_scores=need_scores)
        model_stats = self.model_stats()
        K = self.cnt.shape[0]
        with torch.cuda.device(self.device):
            lab = GF._bank_labels(ids, K, emb.shape[0], self.device)
        return GF.verify_scores_normed(emb, self.models(), self.cnt, self._stats(emb, lab, 0), model_stats, labels=lab,
                                       thresholds=thresholds, need_scores=need_scores)

    def identify(self, emb: torch.Tensor, k: int = 1, ids=None) -> GF.IdentifyOutputs:
        """(R, D) -> the best ``k`` enrolled speakers of every row and their scores; with ``ids`` also the position of each
        row's own speaker among them and the histogram of those positions (`identification_rates` takes it)."""
        return GF.identify(emb, self.models(), self.cnt, k=k, labels=ids)


def eer_from_trial_counts(counts, n_imp: int, n_tgt: int, thresholds=THRESHOLDS):
    """The sweep of `eer_from_labeled_counts` (s5:50-98) over held-out trials: counts (T, 2) = [impostor accepts, target
    accepts], FAR = fa / n_imp, FRR = (n_tgt - ta) / n_tgt; a zero denominator gives 0."""
    n_imp, n_tgt = int(n_imp), int(n_tgt)
    diff, EER, EER_thres, EER_FAR, EER_FRR = 1, 0, 0, 0, 0  # s5:50-54
    for thres, (fa, ta) in zip(thresholds, counts):
        fa, ta = int(fa), int(ta)
        FAR = fa / n_imp if n_imp > 0 else 0
        FRR = (n_tgt - ta) / n_tgt if n_tgt > 0 else 0
        if diff > abs(FAR - FRR):             # s5:93-98
            diff = abs(FAR - FRR)
            EER = (FAR + FRR) / 2
            EER_thres = thres
            EER_FAR = FAR
            EER_FRR = FRR
    return {"EER": EER, "thres": EER_thres, "FAR": EER_FAR, "FRR": EER_FRR}


def evaluate_enrolled(model, enroll_loader, trial_loader, num_speakers: int, device="cuda:0", thresholds=THRESHOLDS,
                      verbose: bool = True, cohort=None, n_top: int = 300):
    """Speaker verification as it is used: both loaders yield (mel, speaker_ids), the ids being bank indices in
    [0, num_speakers).  Every enrolment batch goes into one `SpeakerBank`; every trial batch is scored against it with
    ``need_scores=False`` -- no score matrix is materialised -- and its counts and trial numbers are added on the device in
    int64; ONE read-back at the end.  Returns ONE result over the whole trial set: the dict of `eer_from_trial_counts`
    with ``n_imp`` and ``n_tgt`` added.  ``cohort`` (a `SpeakerBank` of impostor speakers): every trial batch is
    AS-normalised against it over its ``n_top`` best; ``thresholds`` must then be passed, on the normalised scale -- the
    reference's table 0.5 .. 0.99 is one of cosines."""
    if cohort is not None and thresholds is THRESHOLDS:
        raise ValueError("thresholds must be passed with a cohort: the default table is one of cosines, not of normalised scores")
    T = len(thresholds)
    bank = None
    total = None
    with torch.no_grad():
        for mel, speaker_ids in enroll_loader:
            emb = model(mel.to(device)).contiguous().float()
            if bank is None:
                bank = SpeakerBank(num_speakers, emb.shape[1], emb.device)
            bank.enroll(emb, speaker_ids)
        if bank is None:
            raise ValueError("the enrolment loader is empty")
        thr = torch.tensor(list(thresholds), dtype=torch.float64).to(torch.float32)
        if bool((thr[1:] < thr[:-1]).any()):
            raise ValueError("thresholds must be non-decreasing")
        thr = thr.to(bank.device)              # uploaded once: a device table is taken as it is
        if cohort is not None:
            bank.set_cohort(cohort, n_top=n_top)
        for mel, speaker_ids in trial_loader:
            emb = model(mel.to(device)).contiguous().float()
            out = bank.verify(emb, speaker_ids, thresholds=thr, need_scores=False, normalize=cohort is not None)
            part = torch.cat([out.counts.reshape(-1), out.trials]).to(torch.int64)
            total = part if total is None else total + part
    back = total.cpu().numpy() if total is not None else [0] * (2 * T + 2)   # the one read-back
    n_imp, n_tgt = int(back[2 * T]), int(back[2 * T + 1])
    r = eer_from_trial_counts([(back[2 * t], back[2 * t + 1]) for t in range(T)], n_imp, n_tgt, thresholds)
    r["n_imp"], r["n_tgt"] = n_imp, n_tgt
    if verbose:
        print("\nEER : %0.2f (thres:%0.2f, FAR:%0.2f, FRR:%0.2f)" % (r["EER"], r["thres"], r["FAR"], r["FRR"]))
    return r


# ---- identification: who is this row?  (ge2e_identify) ---------------------------------------------------------------------

def identification_rates(hist):
    """hist (k + 1,) of `functional.identify` (or a sum of them) -> the cumulative top-1 .. top-k identification rates,
    cumsum(hist[:k]) / hist.sum(): the share of the rows with a target whose target stands among the first j.  A zero
    denominator gives 0."""
    h = [int(v) for v in (hist.tolist() if hasattr(hist, "tolist") else hist)]
    total, run, rates = sum(h), 0, []
    for v in h[:-1]:
        run += v
        rates.append(run / total if total > 0 else 0)
    return rates


def evaluate_identification(model, enroll_loader, trial_loader, num_speakers: int, k: int = 5, device="cuda:0",
                            verbose: bool = True):
    """Closed- or open-set identification over two loaders, in `evaluate_enrolled`'s shape: both yield (mel, speaker_ids),
    the ids being bank indices in [0, num_speakers).  Every enrolment batch goes into one `SpeakerBank`; every trial batch
    is identified against it, its ``hist`` added on the device in int64; ONE read-back at the end.  Returns ONE result
    over the whole trial set: {"rates": top-1 .. top-k, "hist": [...], "n_tgt": rows with an enrolled target}."""
    bank = None
    total = None
    with torch.no_grad():
        for mel, speaker_ids in enroll_loader:
            emb = model(mel.to(device)).contiguous().float()
            if bank is None:
                bank = SpeakerBank(num_speakers, emb.shape[1], emb.device)
            bank.enroll(emb, speaker_ids)
        if bank is None:
            raise ValueError("the enrolment loader is empty")
        for mel, speaker_ids in trial_loader:
            emb = model(mel.to(device)).contiguous().float()
            part = bank.identify(emb, k=k, ids=speaker_ids).hist.to(torch.int64)
            total = part if total is None else total + part
    hist = [int(v) for v in total.cpu().numpy()] if total is not None else [0] * (int(k) + 1)   # the one read-back
    r = {"rates": identification_rates(hist), "hist": hist, "n_tgt": sum(hist)}
    if verbose:
        print("\ntop-1 : %0.4f   top-%d : %0.4f   (%d trials)" % (r["rates"][0], len(r["rates"]), r["rates"][-1], r["n_tgt"]))
    return r
