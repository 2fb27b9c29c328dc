"""numpy restatement of kgat_eval_rank_f32 / kgat_eval_rank_metrics (include/kgat_hip.h) for the tests: exact ranks of
the held-out items by COUNTING over a score matrix, and the metrics that follow from them.  test_eval_rank_host.py
checks it against brute force (a stable descending argsort and the metrics' definitions)."""
import numpy as np


def masked_scores(score, train, mode):
    """s'(u, i): `score` (users in the order of `train`'s rows x items) with the training items of the mask rule at
    0.0 (reference metric.py:50); unchanged under `drop`."""
    s = np.array(score, dtype=np.float64)
    if mode == "mask":
        for r, tr in enumerate(train):
            s[r, np.asarray(tr, dtype=np.int64)] = 0.0
    return s


def rank_items(score, train, test, mode="mask"):
    """`score` (n_users, n_items) raw scores, `train` / `test` lists of item-position arrays per user (row order).
    Returns one int64 array per user: `above` for the user's test entries in ASCENDING position order, duplicates kept
    (the order of EvalPlan's test CSR); -1 under `drop` for a test entry that is a training item."""
    assert mode in ("mask", "drop")
    s = masked_scores(score, train, mode)
    n_items = s.shape[1]
    pos = np.arange(n_items)
    out = []
    for r in range(s.shape[0]):
        tr = np.unique(np.asarray(train[r], dtype=np.int64))
        cand = np.ones(n_items, dtype=bool)
        if mode == "drop":
            cand[tr] = False
        te = np.sort(np.asarray(test[r], dtype=np.int64))
        a = np.zeros(len(te), dtype=np.int64)
        for j, t in enumerate(te):
            if not cand[t]:
                a[j] = -1
                continue
            before = (s[r] > s[r, t]) | ((s[r] == s[r, t]) & (pos < t))
            a[j] = int((before & cand).sum())
        out.append(a)
    return out


def rank_metrics(above, test, n_candidates, ks):
    """`above` / `test`: per user the counts of rank_items and the test positions (any order; sorted here).  Returns
    (at_k, scalar): (n_users, len(ks), 4) recall / ndcg / precision / hit ratio and (n_users, 4) mrr / ap / auc /
    mean rank, float64, sums in ascending rank order."""
    n_users = len(above)
    at_k = np.zeros((n_users, len(ks), 4))
    scalar = np.zeros((n_users, 4))
    for r in range(n_users):
        te = np.sort(np.asarray(test[r], dtype=np.int64))
        a = np.asarray(above[r], dtype=np.int64)
        first = np.ones(len(te), dtype=bool)
        first[1:] = te[1:] != te[:-1]
        a = np.sort(a[first & (a >= 0)])
        T, C = len(a), int(n_candidates[r])
        for j, k in enumerate(ks):
            hits = a[a < k]
            dcg = 0.0
            for x in hits:
                dcg += 1.0 / np.log2(x + 2.0)
            ideal = 0.0
            for x in range(len(hits)):
                ideal += 1.0 / np.log2(x + 2.0)
            at_k[r, j] = (len(hits) / len(te) if len(te) else 0.0, dcg / ideal if ideal > 0 else 0.0, len(hits) / k,
                          1.0 if len(hits) else 0.0)
        if T:
            ap = 0.0
            for j, x in enumerate(a):
                ap += (j + 1.0) / (x + 1.0)
            gap = int((a - np.arange(T)).sum())
            scalar[r] = (1.0 / (a[0] + 1.0), ap / T, 1.0 - gap / (float(T) * float(C - T)) if C > T else 0.0,
                         float((a + 1).sum()) / T)
    return at_k, scalar
