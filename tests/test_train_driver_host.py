"""What the models and examples/train_kgat.py state once, without a GPU: the top-K of unseen items from a block score
function (metrics.topk_unseen) against brute force, the pretrained-row loader (ckg_io.load_pretrained_rows) through every
class that uses it, and the epoch driver with a stub model on the CPU - its draws, its records and its --log_json file."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import dgl_kgat_amd as K  # noqa: E402
from dgl_kgat_amd import metrics  # noqa: E402


# ------------------------------------------------------------------------------------------------ unseen top-K
N_USERS, N_ITEMS = 7, 11


def _scores():
    """Distinct scores: a permutation of 0 .. 76, scaled (torch.topk promises nothing on ties)."""
    perm = torch.randperm(N_USERS * N_ITEMS, generator=torch.Generator().manual_seed(3))
    S = (perm.double() * 0.125 - 4.0).reshape(N_USERS, N_ITEMS)
    assert torch.unique(S).numel() == S.numel()
    return S


def _plan(train, n_items=N_ITEMS):
    test = {u: np.array([u % n_items]) for u in range(N_USERS)}
    return metrics.EvalPlan(train, test, np.arange(N_USERS, N_USERS + n_items), torch.device("cpu"))


def _train_lists(K_):
    """User 2 has no training item, user 4 exactly n_items - K of them; the others one to three."""
    rng = np.random.default_rng(K_)
    train = {u: rng.permutation(N_ITEMS)[:1 + u % 3] for u in range(N_USERS) if u != 2}
    train[4] = rng.permutation(N_ITEMS)[:N_ITEMS - K_]
    return train


@pytest.mark.parametrize("K_", [1, 3, 11])
def test_topk_unseen_equals_brute_force(K_):
    S = _scores()
    train = {} if K_ == N_ITEMS else _train_lists(K_)       # at K = n_items nobody may have trained on anything
    plan = _plan(train)
    want = []
    for u in range(N_USERS):
        unseen = [i for i in range(N_ITEMS) if i not in set(np.asarray(train.get(u, ())).tolist())]
        want.append(sorted(unseen, key=lambda i: -float(S[u, i]))[:K_])
    if K_ != N_ITEMS:
        assert len(train[4]) == N_ITEMS - K_ and 2 not in train
    blocks = []

    def scores(users, max_bytes):
        blocks.append(users.numel())
        return S[users].clone()

    for max_bytes, sizes in ((1, [1] * N_USERS), (1 << 28, [N_USERS])):
        del blocks[:]
        top = metrics.topk_unseen(scores, N_ITEMS, plan, K_, max_bytes)
        assert blocks == sizes
        assert top.dtype == torch.int32 and top.tolist() == want
    assert torch.equal(S, _scores())                        # the caller's matrix is not written


def test_topk_unseen_refusals():
    S = _scores()
    scores = lambda users, max_bytes: S[users].clone()      # noqa: E731
    plan = _plan(_train_lists(3))
    for bad_K in (0, N_ITEMS + 1):
        with pytest.raises(ValueError):
            metrics.topk_unseen(scores, N_ITEMS, plan, bad_K)
    with pytest.raises(ValueError):
        metrics.topk_unseen(scores, N_ITEMS, _plan({}, n_items=10), 3)


# ------------------------------------------------------------------------------------------------ pretrained rows
def _models():
    n, d = 20, 8
    feats = K.FeatureSets.from_kg(np.array([[5, 0, 14], [6, 1, 15]]), (5, 14), n)
    return (("KGATPropagation", K.KGATPropagation(n, 3, d, d, 1, d, dropout=0.0), "entity_embed"),
            ("CFKG", K.CFKG(n, 3, dim=d), "entity_embed"),
            ("CKE", K.CKE(n, 3, dim=d, relation_dim=d), "cf_embed"),
            ("FM", K.FM(n, feats, dim=d), "embed"),
            ("NFM", K.NFM(n, feats, dim=d, layers=(d,)), "embed"))


def test_load_pretrained_rows_through_every_model():
    n_users, n_items, n = 5, 9, 20
    rng = np.random.default_rng(1)
    ue, ie = rng.standard_normal((n_users, 8)).astype(np.float32), rng.standard_normal((n_items, 8)).astype(np.float32)
    for name, m, attr in _models():
        table = getattr(m, attr).weight
        assert tuple(table.shape) == (n, 8), name
        for as_tensor in (False, True):
            with torch.no_grad():
                for p in m.parameters():
                    p.normal_()
            before = {k: p.detach().clone() for k, p in m.named_parameters()}
            m.load_pretrained(*((torch.as_tensor(ue), torch.as_tensor(ie)) if as_tensor else (ue, ie)), n_users)
            w = table.detach()
            assert np.array_equal(w[:n_users].numpy(), ue) and np.array_equal(w[n_users:n_users + n_items].numpy(), ie), name
            assert torch.equal(w[n_users + n_items:], before[attr + ".weight"][n_users + n_items:]), name
            for k, p in m.named_parameters():
                assert k == attr + ".weight" or torch.equal(p, before[k]), (name, k)
        kept = table.detach().clone()
        for bad in ((ue[:, :4], ie[:, :4], n_users), (ue, ie[:, :4], n_users), (ue, ie, n_users + 1), (ue[:3], ie, n_users),
                    (ue, np.zeros((n - n_users + 1, 8), np.float32), n_users), (ue.reshape(-1), ie, n_users)):
            with pytest.raises(ValueError):
                m.load_pretrained(*bad)
        assert torch.equal(table.detach(), kept), name       # a refused input writes nothing


def test_link_prediction_and_long_are_stated_once():
    from dgl_kgat_amd import fm_models, kg_eval, ripple_models
    for cls in (K.KGATPropagation, K.CFKG, K.CKE):
        assert issubclass(cls, kg_eval.LinkPrediction)
        for name in ("kg_rank", "kg_metrics", "kg_complete"):
            assert name not in vars(cls) and getattr(cls, name) is getattr(kg_eval.LinkPrediction, name)
    assert ripple_models._long is fm_models._long


# ------------------------------------------------------------------------------------------------ the driver
def _train_kgat():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_kgat
    return train_kgat


class _Stub(nn.Module):
    def __init__(self, n_nodes):
        super().__init__()
        self.embed = nn.Embedding(n_nodes, 4)
        self.batches, self.modes = [], []

    def get_loss(self, u, p, n):
        self.batches.append((u.clone(), p.clone(), n.clone()))
        self.modes.append(self.training)
        e = self.embed.weight
        eu = e[u.long()]
        return -F.logsigmoid((eu * e[p.long()]).sum(1) - (eu * e[n.long()]).sum(1)).mean()


def test_driver_on_the_cpu_with_a_stub_model(tmp_path, capsys):
    tk = _train_kgat()
    n_users, n_items, seed = 6, 10, 7
    rng = np.random.default_rng(0)
    cells = rng.permutation(n_users * n_items)
    uv = np.stack([cells // n_items, n_users + cells % n_items], 1).astype(np.int32)
    ds = types.SimpleNamespace(n_users=n_users, n_items=n_items, n_KG_entity=n_users + n_items, n_KG_relation=2,
                               train_pairs=uv[:40], valid_pairs=uv[40:50], test_pairs=uv[50:],
                               item_id_range=np.arange(n_users, n_users + n_items))
    log = str(tmp_path / "log.json")
    args = tk.parse_args(["--epochs", "2", "--max_iters", "3", "--batch_size", "16", "--eval_before", "--seed", str(seed),
                          "--log_json", log])
    dev = torch.device("cpu")
    model = _Stub(n_users + n_items)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    evaluated = []

    def eval_inputs():
        evaluated.append(model.training)
        return {"recall": np.array([0.25]), "ndcg": np.array([0.5])}, {"recall": np.array([0.125]), "ndcg": np.array([0.75])}

    drv = tk.Driver(args, ds, dev)
    fam = tk.Family(model, [lambda epoch, rec: drv.cf_phase(epoch, rec, opt, model.get_loss)], eval_inputs, None)
    torch.manual_seed(seed)
    history = drv.run(fam)
    drv.write_log(fam, history)

    # the parent's draw sequence, restated: per epoch the row indices, then the negatives as int32
    torch.manual_seed(seed)
    pairs = torch.as_tensor(uv[:40])
    want = []
    for _ in range(2):
        n_it, bs = min(40 // 16 + 1, 3), min(16, 40)
        idx = torch.randint(0, 40, (n_it, bs), device=dev)
        neg = torch.randint(n_users, n_users + n_items, (n_it, bs), device=dev, dtype=torch.int32)
        want += [(pairs[idx[i], 0], pairs[idx[i], 1], neg[i]) for i in range(n_it)]
    assert len(model.batches) == len(want) == 6
    for got, exp in zip(model.batches, want):
        for a, b in zip(got, exp):
            assert a.dtype == torch.int32 and torch.equal(a, b)
    assert all(model.modes) and evaluated == [False, False, False]      # phases in training mode, evaluation in eval mode

    evals = {"valid_recall": 0.25, "valid_ndcg": 0.5, "test_recall": 0.125, "test_ndcg": 0.75}
    assert [r["epoch"] for r in history] == [0, 1, 2]
    assert set(history[0]) == {"epoch", "eval_s"} | set(evals)
    for rec in history[1:]:
        assert set(rec) == {"epoch", "cf_s", "cf_iters", "cf_loss", "eval_s", "epoch_s"} | set(evals)
        assert rec["cf_iters"] == 3 and np.isfinite(rec["cf_loss"])
    for rec in history:
        assert {k: rec[k] for k in evals} == evals
    with open(log) as f:
        written = json.load(f)
    assert list(written) == ["args", "n_users", "n_items", "n_entities", "n_relations", "n_train_pairs", "epochs"]
    assert written["epochs"] == history and written["n_train_pairs"] == 40 and written["args"]["max_iters"] == 3
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == "Epoch 0000 | (untrained)" and lines[1] == "           | valid recall@20 0.25000 ndcg@20 0.50000"
    assert [ln[:15] for ln in lines if ln.startswith("Epoch")] == ["Epoch 0000 | (u", "Epoch 0001 | CF", "Epoch 0002 | CF"]


def test_driver_pieces_exist_once():
    """The reading aid of the driver's shape: one clock, one cap, one plan builder, one step loop, one metric line and one
    log writer in the script."""
    with open(os.path.join(ROOT, "examples", "train_kgat.py")) as f:
        text = f.read()
    for piece in ("def cap(", "def clock(", "EvalPlan(", "opt.zero_grad()", "precision@%d", "json.dump(", "torch.randint(0, n_pairs",
                  "torch.randint(0, n_trip"):
        assert text.count(piece) == 1, piece
