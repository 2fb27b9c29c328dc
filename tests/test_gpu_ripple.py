"""Ripple-set attention (csrc/kgat_ripple.hip) and RippleNet on the device: exact inputs, real inputs against float64
under the "10 x the fp32 reference's own error" bar, large logits, bitwise reproducibility, every element written
between intact guard bands, the entries' refusals, the model's loss and gradients, and the planted-structure run.

Graph of the operator tests: 300 nodes, 40 users, two hops, n_rel in {1, 5, 41}; user 0's sets are M copies of one
triple, user 1's relations are all equal, user 2's all different (as far as n_rel allows)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
N_NODES, N_USERS, N_HOP = 300, 40, 2
DIMS, MEMS, SAMPLES, RELS = (16, 32, 64, 128), (1, 2, 5, 32, 33, 128), (1, 3, 257), (1, 5, 41)
NAMES = ("o", "p", "gl", "grad_U", "grad_ent")
_sets = {}


def make_sets(n_rel, M):
    import dgl_kgat_amd as K
    if (n_rel, M) not in _sets:
        rng = np.random.default_rng(1000 * n_rel + M)
        h, t = (rng.integers(0, N_NODES, (N_USERS, N_HOP, M)) for _ in range(2))
        r = np.sort(rng.integers(0, n_rel, (N_USERS, N_HOP, M)), axis=2)
        for x in (h, r, t):
            x[0] = x[0, :, :1]                         # user 0: M copies of one triple
        r[1] = n_rel - 1                               # user 1: one relation
        r[2] = np.sort(np.arange(M) % n_rel)           # user 2: every slot another relation (n_rel >= M), else a cycle
        _sets[(n_rel, M)] = K.RippleSets(h, r, t, N_NODES, n_rel, device=DEV)
    return _sets[(n_rel, M)]


def pick_users(b, seed):
    g = torch.Generator().manual_seed(seed)
    if b == 1:
        return torch.tensor([[0, 1, 2, 7][seed % 4]], dtype=torch.int32)
    if b == 3:
        return torch.tensor([2, 5 + seed % 30, 2], dtype=torch.int32)              # a repeated user
    users = torch.randint(0, N_USERS, (b,), generator=g, dtype=torch.int32)        # 257 draws from 40: repeats
    users[:6] = torch.tensor([0, 1, 2, 0, 1, 2], dtype=torch.int32)
    return users


def restated(ent, U, sets, users, hop, g_o):
    """The five tensors in torch operators, in ent's dtype on ent's device: o, p and, for the loss sum(o * g_o), the
    gradients towards the logits, U and ent."""
    from dgl_kgat_amd.autograd import ripple_hop_torch
    ent, U = ent.detach().clone().requires_grad_(True), U.detach().clone().requires_grad_(True)
    o, p = ripple_hop_torch(ent, U, sets, users, hop, want_p=True)
    grad_ent, grad_U = torch.autograd.grad((o * g_o).sum(), (ent, U))
    sets = sets.to(ent.device)
    T = ent.detach()[sets.mem_t[users.long().to(ent.device), hop].long()]
    gp = (T * g_o.unsqueeze(1)).sum(-1)
    p = p.detach()
    gl = p * (gp - (p * gp).sum(1, keepdim=True))
    return dict(o=o.detach(), p=p, gl=gl, grad_U=grad_U, grad_ent=grad_ent)


def kernels(ent, U, sets, users, hop, g_o):
    from dgl_kgat_amd import ops
    o, p = ops.ripple_hop_fwd(ent, U, sets, users, hop)
    grad_U, gl = ops.ripple_hop_bwd(ent, U, sets, users, hop, p, g_o)
    grad_ent = ops.ripple_scatter(U, sets, users, hop, p, gl, g_o)
    return dict(o=o, p=p, gl=gl, grad_U=grad_U, grad_ent=grad_ent)


def real_inputs(d, M, b, n_rel, reach, seed):
    """float64 ent, U, g_o with the largest |logit| over both hops equal to `reach`."""
    sets = make_sets(n_rel, M).to("cpu")
    g = torch.Generator().manual_seed(seed)
    users = pick_users(b, seed)
    ent = torch.randn(N_NODES, d, dtype=torch.float64, generator=g)
    U = torch.randn(b, n_rel, d, dtype=torch.float64, generator=g)
    g_o = torch.randn(b, d, dtype=torch.float64, generator=g)
    top = 0.0
    for hop in range(N_HOP):
        h, r = sets.mem_h[users.long(), hop].long(), sets.mem_r[users.long(), hop].long()
        s = (ent[h] * U[torch.arange(b).unsqueeze(1), r]).sum(-1)
        top = max(top, float(s.abs().max()))
    return ent, U * (reach / top), g_o, users


def err(x, x64):
    scale = float(x64.abs().max())
    diff = float((x.detach().cpu().double() - x64).abs().max())
    return diff / scale if scale > 0 else diff


def check_against_float64(d, M, b, n_rel, reach, seed):
    """Both hops; returns the worst err(kernel) / bar per tensor."""
    ent, U, g_o, users = real_inputs(d, M, b, n_rel, reach, seed)
    sets = make_sets(n_rel, M)
    worst = dict.fromkeys(NAMES, 0.0)
    for hop in range(N_HOP):
        want = restated(ent, U, sets.to("cpu"), users, hop, g_o)
        cpu32 = restated(ent.float(), U.float(), sets.to("cpu"), users, hop, g_o.float())
        got = kernels(ent.float().to(DEV), U.float().to(DEV).contiguous(), sets, users.to(DEV), hop, g_o.float().to(DEV))
        for name in NAMES:
            assert torch.isfinite(got[name]).all(), (name, d, M, b, n_rel, hop)
            e_k, e_c = err(got[name], want[name]), err(cpu32[name], want[name])
            bar = max(10.0 * e_c, (d + M) * 2.0 ** -24)
            print("d=%d M=%d b=%d n_rel=%d hop=%d %-8s kernel %.3e cpu-fp32 %.3e bar %.3e" % (d, M, b, n_rel, hop, name, e_k, e_c, bar))
            assert e_k <= bar, (name, d, M, b, n_rel, hop, e_k, e_c)
            worst[name] = max(worst[name], e_k / bar)
    return worst


def grid_case(d, M):
    """The (n_samples, n_rel) pairs of one (d, M): every n_samples, the relations rotating with the case."""
    k = DIMS.index(d) * len(MEMS) + MEMS.index(M)
    return [(b, RELS[(k + j) % 3]) for j, b in enumerate(SAMPLES)]


# ------------------------------------------------------------------------------------------------ 1. exact inputs
@pytest.mark.parametrize("M", [2, 32, 128])
@pytest.mark.parametrize("d", DIMS)
def test_exact_inputs_give_exact_outputs(d, M):
    """U = 0 and M a power of two: p = 1 / M exactly; tail rows in {-1, -1/2, 0, 1/2, 1}: o is the float64 mean bit for
    bit; g_o with 8 non-zero columns of the same values: every sum of the backward is exact in fp32 (gp a multiple of
    1/4 up to 8, gl of 1 / (4 M^2) up to 16 / M, grad_U of 1 / (8 M^2) up to 16: at most 22 bits), so gl, grad_U and
    grad_ent equal float64 bit for bit."""
    b, n_rel = 257, RELS[(DIMS.index(d) + M) % 3]
    sets = make_sets(n_rel, M)
    g = torch.Generator().manual_seed(d + M)
    users = pick_users(b, d + M)
    ent = torch.randint(-2, 3, (N_NODES, d), generator=g).double() / 2
    U = torch.zeros(b, n_rel, d, dtype=torch.float64)
    g_o = torch.randint(-2, 3, (b, d), generator=g).double() / 2
    keep = torch.zeros(b, d, dtype=torch.bool)
    keep.scatter_(1, torch.rand(b, d, generator=g).argsort(1)[:, :8], True)
    g_o = g_o * keep
    for hop in range(N_HOP):
        want = restated(ent, U, sets.to("cpu"), users, hop, g_o)
        got = kernels(ent.float().to(DEV), U.float().to(DEV), sets, users.to(DEV), hop, g_o.float().to(DEV))
        assert torch.equal(got["p"].cpu(), torch.full((b, M), 1.0 / M))
        assert want["gl"].abs().max() > 0 and want["grad_U"].abs().max() > 0
        for name in NAMES:
            assert torch.equal(got[name].cpu().double(), want[name]), (name, d, M, hop)


# ------------------------------------------------------------------------------------------------ 2. real inputs
@pytest.mark.parametrize("M", MEMS)
@pytest.mark.parametrize("d", DIMS)
def test_real_inputs_against_float64(d, M):
    """Logits within +-4, both hops, n_samples in {1, 3, 257}: for each of o, p, gl, grad_U and grad_ent,
    err(x) = max|x - x64| / max|x64| against the float64 restatement, and
    err(kernel) <= max(10 x err(CPU fp32 restatement), (d + M) 2^-24).
    Measured on MI355X, the worst err(kernel) / bar over the grid: see DESIGN.md section 28."""
    for b, n_rel in grid_case(d, M):
        worst = check_against_float64(d, M, b, n_rel, 4.0, 7 * d + M + b)
        print("worst fraction of the bar d=%d M=%d b=%d n_rel=%d: %s" % (d, M, b, n_rel, {k: "%.3f" % v for k, v in worst.items()}))


# ------------------------------------------------------------------------------------------------ 3. large logits
@pytest.mark.parametrize("d,M,n_rel", [(16, 5, 41), (16, 128, 5), (128, 5, 1), (128, 128, 41), (64, 33, 5)])
def test_large_logits_stay_finite(d, M, n_rel):
    """|s| reaches 100: without the subtracted maximum exp overflows.  Finite, and the bar of the real inputs."""
    check_against_float64(d, M, 257, n_rel, 100.0, d + M)


# ------------------------------------------------------------------------------------------------ 4. reproducibility
@pytest.mark.parametrize("d,M,n_rel", [(16, 33, 5), (32, 128, 1), (64, 32, 41), (128, 128, 5)])
def test_bitwise_reproducible(d, M, n_rel):
    ent, U, g_o, users = real_inputs(d, M, 257, n_rel, 4.0, 3)
    sets = make_sets(n_rel, M)
    args = (ent.float().to(DEV), U.float().to(DEV).contiguous(), sets, users.to(DEV), 1, g_o.float().to(DEV))
    a, b = kernels(*args), kernels(*args)
    for name in NAMES:
        assert torch.equal(a[name].view(torch.int32), b[name].view(torch.int32)), name


# ------------------------------------------------------------------------------------------------ 5. every element written
GUARD = 1024          # floats: 4 KB on each side


def carved(n, fill):
    buf = torch.full((n + 2 * GUARD,), -12345.0, dtype=torch.float32, device=DEV)
    out = buf[GUARD:GUARD + n]
    out.fill_(fill)
    return buf, out


def bands_intact(buf, n):
    return bool((buf[:GUARD] == -12345.0).all()) and bool((buf[GUARD + n:] == -12345.0).all())


@pytest.mark.parametrize("d,M,n_rel,b", [(16, 5, 41, 257), (32, 1, 41, 3), (64, 32, 5, 257), (128, 128, 1, 3), (64, 33, 41, 1)])
def test_every_element_is_written_between_intact_bands(d, M, n_rel, b):
    from dgl_kgat_amd import _lib
    lib = _lib.load()
    ent, U, g_o, users = real_inputs(d, M, b, n_rel, 4.0, 9)
    sets = make_sets(n_rel, M)
    ent, U, g_o, users = ent.float().to(DEV), U.float().to(DEV).contiguous(), g_o.float().to(DEV), users.to(DEV)
    nan = float("nan")
    bufs = {"o": carved(b * d, nan), "p": carved(b * M, nan), "grad_U": carved(b * n_rel * d, nan), "gl": carved(b * M, nan)}
    stream = torch.cuda.current_stream().cuda_stream
    statics = (b, d, M, n_rel, N_HOP, 1, N_NODES, N_USERS, ent.data_ptr(), U.data_ptr(), sets.mem_h.data_ptr(),
               sets.mem_r.data_ptr(), sets.mem_t.data_ptr(), users.data_ptr())
    assert lib.kgat_ripple_hop_fwd_f32(*statics, bufs["o"][1].data_ptr(), bufs["p"][1].data_ptr(), stream) == 0
    assert lib.kgat_ripple_hop_bwd_f32(*statics, bufs["p"][1].data_ptr(), g_o.data_ptr(), bufs["grad_U"][1].data_ptr(),
                                       bufs["gl"][1].data_ptr(), stream) == 0
    torch.cuda.synchronize()
    for name, (buf, out) in bufs.items():
        assert not torch.isnan(out).any(), name
        assert bands_intact(buf, out.numel()), name
    # the rows of grad_U for relations a sample's set lacks: +0.0, written
    gU = bufs["grad_U"][1].view(b, n_rel, d)
    r = sets.mem_r[users.long(), 1].long()
    present = torch.zeros(b, n_rel, dtype=torch.bool, device=DEV)
    present[torch.arange(b, device=DEV).unsqueeze(1), r] = True
    absent = gU[~present]
    assert (n_rel == 1 or absent.numel() > 0) and bool((absent == 0).all()) and not bool(torch.signbit(absent).any())
    assert M == 1 or bool(gU[present].abs().sum() > 0)          # (one slot: p = 1 and the logit's gradient is 0)


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_entry_refusals_and_a_bad_user_id():
    from test_ripple_host import BADARG, ENTRIES, UNSUPPORTED, call_entry
    from dgl_kgat_amd import ops
    for entry, word in ENTRIES.items():
        for sizes, code in ((dict(d=24), UNSUPPORTED), (dict(n_memory=129), UNSUPPORTED), (dict(hop=2), BADARG), (dict(hop=-1), BADARG)):
            rc, msg = call_entry(entry, sizes)
            assert rc == code and "ripple" in msg and word in msg, (entry, sizes, rc, msg)
    d, M, n_rel, b = 32, 5, 5, 7
    ent, U, g_o, users = real_inputs(d, M, b, n_rel, 4.0, 1)
    sets = make_sets(n_rel, M)
    ent, U, g_o = ent.float().to(DEV), U.float().to(DEV).contiguous(), g_o.float().to(DEV)
    with pytest.raises(ops.KGATLibraryError, match="ripple"):
        ops.ripple_hop_fwd(ent, U, sets, users.to(DEV), 2)
    with pytest.raises(ops.KGATLibraryError, match="aligned"):
        ops.ripple_hop_fwd(torch.zeros(N_NODES * d + 1, device=DEV)[1:].view(N_NODES, d), U, sets, users.to(DEV), 0)
    with pytest.raises(ops.KGATLibraryError, match="null"):
        _lib_null_users(ent, U, sets, b)
    good = kernels(ent, U, sets, users.to(DEV), 0, g_o)
    bad = users.clone()
    bad[2], bad[5] = N_USERS, -1
    o, p = ops.ripple_hop_fwd(ent, U, sets, bad.to(DEV), 0)
    grad_U, gl = ops.ripple_hop_bwd(ent, U, sets, bad.to(DEV), 0, p, g_o)
    torch.cuda.synchronize()
    rows = torch.tensor([i not in (2, 5) for i in range(b)], device=DEV)
    for got, name in ((o, "o"), (p, "p"), (grad_U, "grad_U"), (gl, "gl")):
        assert bool(torch.isnan(got[~rows]).all()), name                  # NaN for that sample ...
        assert torch.equal(got[rows], good[name][rows]), name            # ... and for that sample only


def _lib_null_users(ent, U, sets, b):
    """The forward with a null `users`: refused by the entry, reported through ops.check."""
    from dgl_kgat_amd import _lib
    lib = _lib.load()
    o = torch.empty(b, ent.shape[1], device=DEV)
    p = torch.empty(b, sets.n_memory, device=DEV)
    rc = lib.kgat_ripple_hop_fwd_f32(b, ent.shape[1], sets.n_memory, sets.n_rel, sets.n_hop, 0, sets.n_nodes, sets.n_users,
                                     ent.data_ptr(), U.data_ptr(), sets.mem_h.data_ptr(), sets.mem_r.data_ptr(),
                                     sets.mem_t.data_ptr(), None, o.data_ptr(), p.data_ptr(), None)
    _lib.check(rc, "kgat_ripple_hop_fwd_f32")


# ------------------------------------------------------------------------------------------------ 7. autograd, the model
_planted = {}


def planted_small():
    """The 200-user / 150-item planted CKG (examples/train_kgat.planted_data_dir) and its ripple sets, built once."""
    if not _planted:
        sys.path.insert(0, os.path.join(ROOT, "examples"))
        import train_kgat
        import dgl_kgat_amd as K
        ds = K.CKGDataset(train_kgat.planted_data_dir(n_users=200, n_items=150, n_attrs=12, per_user=12, seed=7))
        _planted["ds"] = ds
        _planted["sets"] = K.RippleSets.build(ds.train_KG_triplet, ds.train_pairs, ds.n_users, ds.n_KG_entity, n_hop=2,
                                              n_memory=32, seed=7, add_inverse=True)
    return _planted["ds"], _planted["sets"]


@pytest.mark.parametrize("d", [16, 64])
def test_loss_and_parameter_gradients_through_the_model(d):
    """RippleNet.get_loss (both hops, the KGE and L2 terms) on the planted 200 x 150 CKG, batch 256: the device model on
    autograd.ripple_hop against the same model in float64 on ripple_hop_torch; the loss and every parameter gradient
    within the bar of the real inputs, err <= max(10 x err(CPU fp32 model), (d + M) 2^-24)."""
    import dgl_kgat_amd as K
    from dgl_kgat_amd import autograd
    ds, sets = planted_small()
    torch.manual_seed(d)

    def make():
        return K.RippleNet(ds.n_KG_entity, sets, dim=d, kge_weight=0.01, reg_lambda=1e-3, item_range=(ds.n_users, ds.n_users + ds.n_items))
    m = make()
    with torch.no_grad():
        m.entity_emb.weight.mul_(6.0)            # logits of order one: the softmax is not flat
    cpu, ref = make(), make().double()
    cpu.load_state_dict(m.state_dict())
    ref.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    dev = m.to(DEV)
    assert autograd.ripple_kernels_apply(dev.entity_emb.weight, torch.empty(512, sets.n_rel, d, device=DEV), sets)
    g = torch.Generator().manual_seed(5)
    b = 256
    pick = torch.randint(0, len(ds.train_pairs), (b,), generator=g)
    u = torch.as_tensor(ds.train_pairs[:, 0].astype(np.int64))[pick]
    p = torch.as_tensor(ds.train_pairs[:, 1].astype(np.int64))[pick]
    n = torch.randint(ds.n_users, ds.n_users + ds.n_items, (b,), generator=g)
    out = {}
    for name, model, where in (("device", dev, DEV), ("cpu32", cpu, "cpu"), ("ref", ref, "cpu")):
        loss = model.get_loss(u.to(where), p.to(where), n.to(where))
        loss.backward()
        out[name] = (float(loss.detach()), {k: v.grad.detach().cpu().double() for k, v in model.named_parameters()})
    want_loss, want = out["ref"]
    assert abs(out["device"][0] - want_loss) <= max(10 * abs(out["cpu32"][0] - want_loss), (d + 32) * 2.0 ** -24 * abs(want_loss))
    for k, gw in want.items():
        e_k, e_c = err(out["device"][1][k], gw), err(out["cpu32"][1][k], gw)
        bar = max(10.0 * e_c, (d + 32) * 2.0 ** -24)
        print("d=%d %s: device %.3e cpu-fp32 %.3e bar %.3e" % (d, k, e_k, e_c, bar))
        assert gw.abs().max() > 0 and e_k <= bar, (k, e_k, e_c)


# ------------------------------------------------------------------------------------------------ 8. the planted run
# the arguments of test_gpu_fm.test_planted_structure_recall_rises; --lr tuned once, 0.03 -> 0.01 (at 0.03 Adam overshoots
# after the first epoch: the loss rises again)
PLANTED_ARGS = ["--planted", "--epochs", "3", "--lr", "0.01", "--batch_size", "512", "--batch_size_kg", "512", "--eval_before",
                "--seed", "1234"]


def test_planted_structure_recall_rises(capsys):
    """examples/train_kgat.py --model ripplenet --planted --ripple_inverse 1 under the criterion of
    test_gpu_fm.test_planted_structure_recall_rises: untrained test recall@20 inside (0.005, 0.05) - a random ranking -,
    more than 3 x that after the last epoch, the CF loss falling.  Measured on MI355X (test recall@20, untrained then per
    epoch): 0.0180 -> 0.2518, 0.3668, 0.3936 (CF loss 0.4913, 0.2624, 0.1913) at d = 64, M = 32, two hops."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_kgat
    hist = train_kgat.main(["--model", "ripplenet", "--ripple_inverse", "1"] + PLANTED_ARGS)
    rec = [h["test_recall"] for h in hist]
    with capsys.disabled():
        print("\n--model ripplenet planted-structure run: test recall@20 by epoch %s, valid %s, CF loss %s" % (
            ["%.4f" % r for r in rec], ["%.4f" % h["valid_recall"] for h in hist], ["%.4f" % h["cf_loss"] for h in hist[1:]]))
    assert len(hist) == 4 and 0.005 < rec[0] < 0.05                # untrained: a random ranking
    assert rec[3] > 3.0 * rec[0]
    assert hist[3]["cf_loss"] < hist[1]["cf_loss"]
