"""FM and NFM (fm_models.py) on the device: loss and every parameter gradient against float64, FM's dot-product readout
under the evaluation kernel against a torch sort of its own score matrix, and both models end to end on the planted CKG."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
_planted = {}


def planted_small():
    """The 200-user / 150-item planted CKG (examples/train_kgat.planted_data_dir), built once."""
    if not _planted:
        sys.path.insert(0, os.path.join(ROOT, "examples"))
        import train_kgat
        import dgl_kgat_amd as K
        ds = K.CKGDataset(train_kgat.planted_data_dir(n_users=200, n_items=150, n_attrs=12, per_user=12, seed=7))
        _planted["ds"] = ds
        _planted["dicts"] = (train_kgat.user_dict(ds.train_pairs, ds.n_users), train_kgat.user_dict(ds.test_pairs, ds.n_users))
    return _planted["ds"], _planted["dicts"]


def _models(kind, ds, seed):
    import dgl_kgat_amd as K
    items = (ds.n_users, ds.n_users + ds.n_items)
    feats = K.FeatureSets.from_kg(ds.train_KG_triplet, items, ds.n_KG_entity)
    torch.manual_seed(seed)
    make = (lambda: K.FM(ds.n_KG_entity, feats, dim=64, reg_lambda=1e-3)) if kind == "fm" else \
        (lambda: K.NFM(ds.n_KG_entity, feats, dim=64, layers=(64,), dropout=0.0, reg_lambda=1e-3))
    m = make()
    with torch.no_grad():   # every parameter in play: the linear weights and w0 start at zero
        m.w_lin.normal_(0, 0.1)
        m.w0.fill_(0.2)
        m.embed.weight.mul_(4.0)
    ref = make().double()
    ref.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    cpu = m_copy_cpu(make, m)
    return m.to(DEV), cpu, ref


def m_copy_cpu(make, m):
    c = make()
    c.load_state_dict(m.state_dict())
    return c


@pytest.mark.parametrize("kind", ["fm", "nfm"])
def test_loss_and_parameter_gradients_against_float64(kind):
    """get_loss and the gradient of every parameter on the planted 200 x 150 CKG, batch 256 (512 pooled sets, the
    kernels' route), against the float64 torch restatement.

    The bar, from the number format alone.  An element of a gradient is a sum of 2 b contributions - through y_pos and
    through y_neg of each of the b samples, +-sigma_s / b x dy / dtheta, and the regulariser's lambda / (2 b) x dsq / dtheta
    - each itself a short sum: the set's n <= 8 rows, a 64-wide layer forward and backward.  fp32 summation in any order
    is within (number of terms) 2^-24 sum |term| of the exact sum to first order, so an element may be off by
    (2 b + n + 2 x 64 + 16) 2^-24 A, with A the sum of the absolute values of those contributions, taken from float64
    backward passes per pooled set (w0 and a user's w_lin cancel between the two halves of a sample: their A does not).
    Where A = 0 - a table row no set touches - the gradient must be exactly 0.  The loss: a mean of b softplus values
    plus a small regulariser, within (b + 16) 2^-24 of its magnitude.  The same model in fp32 torch operators on the
    CPU is held to the same bars (a bar the comparator itself misses would be no bar).  Prints the worst fraction of the
    bar per tensor."""
    from dgl_kgat_amd import ops
    ds, _ = planted_small()
    dev_m, cpu_m, ref_m = _models(kind, ds, 11)
    g = torch.Generator().manual_seed(5)
    b = 256
    assert ops.bi_pool_supported(64, 2 * b)
    pick = torch.randint(0, len(ds.train_pairs), (b,), generator=g)
    u = torch.as_tensor(ds.train_pairs[:, 0].astype(np.int64))[pick]
    p = torch.as_tensor(ds.train_pairs[:, 1].astype(np.int64))[pick]
    n = torch.randint(ds.n_users, ds.n_users + ds.n_items, (b,), generator=g)
    out = {}
    for name, m, where in (("device", dev_m, DEV), ("cpu32", cpu_m, "cpu"), ("ref", ref_m, "cpu")):
        loss = m.get_loss(u.to(where), p.to(where), n.to(where))
        loss.backward()
        out[name] = (float(loss.detach()), {k: v.grad.detach().cpu().double().numpy() for k, v in m.named_parameters()})
    want_loss, want = out["ref"]
    A = {k: np.zeros_like(v) for k, v in want.items()}
    names, params = zip(*ref_m.named_parameters())
    for s_ in range(b):
        halves = []
        for item in (p[s_:s_ + 1], n[s_:s_ + 1]):
            bi, lin, sq = ref_m.pool(u[s_:s_ + 1], item)
            y = (ref_m.w0 + lin + ref_m._head(bi)).sum()
            gy = torch.autograd.grad(y, params, retain_graph=True, allow_unused=True)
            gq = torch.autograd.grad(sq.sum(), params, allow_unused=True)
            halves.append((float(y.detach()), gy, gq))
        sigma = 1.0 / (1.0 + np.exp(-(halves[1][0] - halves[0][0])))
        for _, gy, gq in halves:
            for k, a_, q_ in zip(names, gy, gq):
                if a_ is not None:
                    A[k] += sigma / b * a_.abs().numpy()
                if q_ is not None:
                    A[k] += ref_m.reg_lambda / (2 * b) * q_.abs().numpy()
    n_max = 1 + max(len(x) for x in dev_m.feats.lists())
    assert n_max <= 8
    unit = (2 * b + n_max + 2 * 64 + 16) * 2.0 ** -24
    for who in ("device", "cpu32"):
        got_loss, got = out[who]
        assert abs(got_loss - want_loss) <= (b + 16) * 2.0 ** -24 * abs(want_loss), (who, got_loss, want_loss)
        for k, gw in want.items():
            err = np.abs(got[k] - gw)
            bar = unit * A[k]
            assert A[k].max() > 0 and np.all(err[bar == 0] == 0), (who, k)
            worst = float((err[bar > 0] / bar[bar > 0]).max())
            print("%s %s %s: worst fraction of the bar %.4f" % (kind, who, k, worst))
            assert worst <= 1.0, (who, k, worst)
    # the dense gradient: rows of the table no set touches are exactly zero
    touched = np.zeros(ds.n_KG_entity, bool)
    lists = dev_m.feats.lists()
    for i in torch.cat([p, n]).tolist():
        touched[lists[i - ds.n_users]] = True
    touched[u.numpy()] = True
    assert (~touched).any() and not dev_m.embed.weight.grad.cpu().numpy()[~touched].any()


def test_fm_readout_under_the_evaluation_kernel_is_exact():
    """Integer-valued tables: every score is an integer fp32 holds, through the pooled route and through the readout's
    dot products alike, so calc_recall_ndcg(readout) must equal - exactly - a stable descending torch sort of FM's own
    score matrix with the training items masked to 0.0 (the reference's rule; ties keep the lower item first)."""
    import dgl_kgat_amd as K
    from dgl_kgat_amd import metrics
    ds, (train_dict, test_dict) = planted_small()
    items = (ds.n_users, ds.n_users + ds.n_items)
    feats = K.FeatureSets.from_kg(ds.train_KG_triplet, items, ds.n_KG_entity)
    m = K.FM(ds.n_KG_entity, feats, dim=16).to(DEV)
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        m.embed.weight.copy_(torch.randint(-1, 2, m.embed.weight.shape, generator=g).float())
        m.w_lin.copy_(torch.randint(-2, 3, m.w_lin.shape, generator=g).float())
        m.w0.fill_(3.0)
    table = m.readout((0, ds.n_users), items)
    users = sorted(test_dict)
    uu, ii = torch.meshgrid(torch.as_tensor(users), torch.arange(*items), indexing="ij")
    y = torch.cat([m.score(a.to(DEV), b.to(DEV)).detach() for a, b in zip(uu.reshape(-1).split(8192), ii.reshape(-1).split(8192))])
    y = y.reshape(len(users), ds.n_items)
    assert torch.equal(y, y.round()) and y.abs().max() < 2 ** 20
    dots = table[torch.as_tensor(users, device=DEV)] @ table[items[0]:items[1]].T
    assert torch.equal(dots, y)
    # a torch sort of y, the reference's metric (metric.py:23-34, 50-63)
    K20 = 20
    score = y.clone().double()
    for r, u in enumerate(users):
        score[r, torch.as_tensor(np.asarray(train_dict.get(u, ()), dtype=np.int64), device=DEV)] = 0.0
    top = torch.sort(score, dim=1, descending=True, stable=True).indices[:, :K20].cpu().numpy()
    disc = 1.0 / np.log2(np.arange(2, K20 + 2))
    rec = ndcg = 0.0
    for r, u in enumerate(users):
        hits = np.isin(top[r], test_dict[u]).astype(np.float64)
        rec += hits.sum() / len(test_dict[u])
        ideal = (np.sort(hits)[::-1] * disc).sum()
        ndcg += (hits * disc).sum() / ideal if ideal > 0 else 0.0
    got = metrics.calc_recall_ndcg(table, train_dict, test_dict, ds.item_id_range, K=K20)
    assert abs(got[0] - rec / len(users)) <= 1e-12 and abs(got[1] - ndcg / len(users)) <= 1e-12, (got, rec / len(users), ndcg / len(users))


# the arguments of test_gpu_transe.test_planted_structure_recall_rises
PLANTED_ARGS = ["--planted", "--epochs", "3", "--lr", "0.03", "--batch_size", "512", "--batch_size_kg", "512", "--eval_before",
                "--seed", "1234"]


@pytest.mark.parametrize("model", ["fm", "nfm"])
def test_planted_structure_recall_rises(model, capsys):
    """examples/train_kgat.py --model {fm, nfm} --planted with the arguments and under the criterion of
    test_gpu_transe.test_planted_structure_recall_rises: untrained test recall@20 inside (0.005, 0.05) - a random
    ranking -, more than 3 x that after the last epoch, the CF loss falling.  Measured on MI355X (test recall@20,
    untrained then per epoch) - fm: 0.0254 -> 0.3808, 0.4224, 0.4181 (CF loss 0.4109, 0.1944, 0.1847); nfm: 0.0213 ->
    0.4288, 0.4959, 0.5289 (CF loss 0.4121, 0.1688, 0.1298), with the Xavier tables the models start from."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_kgat
    hist = train_kgat.main(["--model", model] + PLANTED_ARGS)
    rec = [h["test_recall"] for h in hist]
    with capsys.disabled():
        print("\n--model %s planted-structure run: test recall@20 by epoch %s, valid %s, CF loss %s" % (
            model, ["%.4f" % r for r in rec], ["%.4f" % h["valid_recall"] for h in hist], ["%.4f" % h["cf_loss"] for h in hist[1:]]))
    assert len(hist) == 4 and 0.005 < rec[0] < 0.05                # untrained: a random ranking
    assert rec[3] > 3.0 * rec[0]
    assert hist[3]["cf_loss"] < hist[1]["cf_loss"]
