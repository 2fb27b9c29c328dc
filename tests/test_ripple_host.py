"""RippleNet without a GPU: the ripple sets against a brute-force reading of their rule, the torch restatement of the
hop operator against a per-sample float64 loop, the model (update modes, loss terms, the all-pairs scorer against the
per-pair path, the release's parameter names), the new entries' types and refusals (made before any device work: they
come back on a machine without a device) and the harness's arguments."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import dgl_kgat_amd as K  # noqa: E402
from dgl_kgat_amd import _lib, autograd, ripple_models  # noqa: E402

from test_workspace_host import BADARG, OK, P, declarations  # noqa: E402

UNSUPPORTED = -2

# ------------------------------------------------------------------------------------------------ a small CKG
N_USERS, N_NODES, N_KG_REL = 5, 25, 3
USER_ITEMS = {0: [5, 6, 7], 1: [8, 9], 2: [23], 3: [24], 4: [10, 11, 12, 13, 14]}


def small_ckg(user_items=None):
    """Items 5..14 with 1..6 attribute triples each (attributes 15..22, relations 0..2), item 23 without a triple,
    item 24 with one; interaction triples in both directions (relations 3, 4), which the sets must leave out."""
    rng = np.random.default_rng(3)
    trip = set()
    for i in range(5, 15):
        for _ in range(int(rng.integers(1, 7))):
            trip.add((i, int(rng.integers(0, N_KG_REL)), int(rng.integers(15, 23))))
    trip.add((24, 1, 22))
    trip.add((5, 2, 6))                                       # an item -> item triple: hop 2 exists without inverses
    pairs = [(u, i) for u, items in (user_items or USER_ITEMS).items() for i in items]
    both = sorted(trip) + [(u, 3, i) for u, i in pairs] + [(i, 4, u) for u, i in pairs]
    return np.asarray(both, dtype=np.int64), np.asarray(pairs, dtype=np.int64), sorted(trip)


def augmented(kg, inverse):
    return sorted(set(kg) | ({(t, r + N_KG_REL, h) for h, r, t in kg} if inverse else set()))


def brute_sets(kg, items, n_hop, M, seed, user):
    """The rule of RippleSets.build, read literally."""
    out, heads, prev = [], sorted(set(items)), None
    for k in range(1, n_hop + 1):
        cand = [x for x in kg if x[0] in heads]                 # kg is sorted (h, r, t)
        if not cand:
            cur = prev if prev is not None else [(items[0], 0, items[0])] * M
        else:
            pick = np.random.default_rng([seed, user, k]).choice(len(cand), M, replace=len(cand) < M)
            cur = sorted((cand[j] for j in pick), key=lambda x: (x[1], x[0], x[2]))
        out.append(cur)
        heads, prev = sorted({x[2] for x in cur}), cur
    return out


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("M", [4, 32])
def test_ripple_sets_follow_their_rule(inverse, M):
    trip, pairs, kg = small_ckg()
    sets = K.RippleSets.build(trip, pairs, N_USERS, N_NODES, n_hop=3, n_memory=M, seed=11, add_inverse=inverse)
    assert (sets.n_users, sets.n_hop, sets.n_memory, sets.n_nodes) == (N_USERS, 3, M, N_NODES)
    assert sets.n_rel == (2 * N_KG_REL if inverse else N_KG_REL)
    assert sets.mem_h.dtype == torch.int32 and tuple(sets.mem_h.shape) == (N_USERS, 3, M) and sets.to("cpu") is sets
    h, r, t = (getattr(sets, n).numpy() for n in ("mem_h", "mem_r", "mem_t"))
    full = augmented(kg, inverse)
    assert list(sets.valid) == [True, True, False, True, True]
    with_repl = without = copied = 0
    for u, items in USER_ITEMS.items():
        got = [list(zip(h[u, k].tolist(), r[u, k].tolist(), t[u, k].tolist())) for k in range(3)]
        assert got == brute_sets(full, items, 3, M, 11, u), u
        if not sets.valid[u]:
            assert got[0] == [(23, 0, 23)] * M and got[1] == got[0] and got[2] == got[0]     # the fill, copied down
            continue
        heads = set(items)
        for k in range(3):
            assert all(x in full for x in got[k])                              # every stored triple exists
            assert got[k] == sorted(got[k], key=lambda x: (x[1], x[0], x[2]))   # (r, h, t) ascending
            assert (np.diff(r[u, k]) >= 0).all()
            n_cand = sum(1 for x in full if x[0] in heads)
            if n_cand:
                assert {x[0] for x in got[k]} <= heads, (u, k)                 # heads: the items, then the last tails
            if n_cand == 0:
                assert k > 0 and got[k] == got[k - 1]                          # an empty hop copies the one before
                copied += 1
            elif n_cand < M:
                assert len(set(got[k])) < M                                    # with replacement: something repeats
                with_repl += 1
            else:
                assert len(set(got[k])) == M                                   # without: M distinct candidates
                without += 1
            heads = {x[2] for x in got[k]}
    assert with_repl and copied if not inverse else with_repl
    assert without or M == 32


def test_ripple_sets_are_reproducible_and_per_user():
    trip, pairs, _ = small_ckg()
    a = K.RippleSets.build(trip, pairs, N_USERS, N_NODES, n_memory=4, seed=5, add_inverse=True)
    b = K.RippleSets.build(trip, pairs, N_USERS, N_NODES, n_memory=4, seed=5, add_inverse=True)
    c = K.RippleSets.build(trip, pairs, N_USERS, N_NODES, n_memory=4, seed=6, add_inverse=True)
    for n in ("mem_h", "mem_r", "mem_t"):
        assert torch.equal(getattr(a, n), getattr(b, n))
    assert any(not torch.equal(getattr(a, n), getattr(c, n)) for n in ("mem_h", "mem_r", "mem_t"))
    other = dict(USER_ITEMS)
    other[1] = [12, 13, 14, 5]
    trip2, pairs2, _ = small_ckg(other)
    d = K.RippleSets.build(trip2, pairs2, N_USERS, N_NODES, n_memory=4, seed=5, add_inverse=True)
    for n in ("mem_h", "mem_r", "mem_t"):
        x, y = getattr(a, n), getattr(d, n)
        assert all(torch.equal(x[u], y[u]) for u in (0, 2, 3, 4))
    assert not torch.equal(a.mem_h[1], d.mem_h[1])


def test_ripple_sets_refuse():
    trip, pairs, _ = small_ckg()
    for kw in (dict(n_hop=0), dict(n_hop=5), dict(n_memory=0), dict(n_memory=129)):
        with pytest.raises(ValueError):
            K.RippleSets.build(trip, pairs, N_USERS, N_NODES, **kw)
    bad = trip.copy()
    bad[0, 2] = N_NODES
    with pytest.raises(ValueError):
        K.RippleSets.build(bad, pairs, N_USERS, N_NODES)
    bad = trip.copy()
    bad[0, 1] = -1
    with pytest.raises(ValueError):
        K.RippleSets.build(bad, pairs, N_USERS, N_NODES)
    for bad_pair in ([N_USERS, 6], [0, 2], [0, N_NODES]):
        with pytest.raises(ValueError):
            K.RippleSets.build(trip, np.vstack([pairs, [bad_pair]]), N_USERS, N_NODES)
    ok = np.zeros((2, 1, 3), dtype=np.int64)
    K.RippleSets(ok, ok, ok, 4, 2)
    for h, r, t in ((ok + 4, ok, ok), (ok, ok + 2, ok), (ok, ok, ok - 1), (ok, np.array([[[1, 0, 0]], [[0, 0, 0]]]), ok),
                    (ok, ok[:, :, :2], ok), (np.zeros((2, 5, 3), int),) * 3, (np.zeros((2, 1, 129), int),) * 3):
        with pytest.raises(ValueError):
            K.RippleSets(h, r, t, 4, 2)


# ------------------------------------------------------------------------------------------------ the operator
def test_ripple_hop_torch_against_a_float64_loop():
    """12 nodes, 3 relations, M = 5: o and the gradients towards ent and U of sum(o * c), sample by sample."""
    g = torch.Generator().manual_seed(0)
    n, n_rel, M, d, n_users, n_hop = 12, 3, 5, 4, 3, 2
    h = torch.randint(0, n, (n_users, n_hop, M), generator=g)
    t = torch.randint(0, n, (n_users, n_hop, M), generator=g)
    r = torch.sort(torch.randint(0, n_rel, (n_users, n_hop, M), generator=g), dim=2).values
    sets = K.RippleSets(h, r, t, n, n_rel)
    users = torch.tensor([2, 0, 2, 1])
    ent = torch.randn(n, d, dtype=torch.float64, generator=g, requires_grad=True)
    U = torch.randn(4, n_rel, d, dtype=torch.float64, generator=g, requires_grad=True)
    c = torch.randn(4, d, dtype=torch.float64, generator=g)
    for hop in range(n_hop):
        o, p = autograd.ripple_hop_torch(ent, U, sets, users, hop, want_p=True)
        assert K.ripple_hop(ent, U, sets, users, hop).equal(o)          # CPU tensors take the restatement
        ge, gU = torch.autograd.grad((o * c).sum(), (ent, U))
        E, Un = ent.detach().numpy(), U.detach().numpy()
        want_o, want_ge, want_gU = np.zeros((4, d)), np.zeros((n, d)), np.zeros((4, n_rel, d))
        for b, u in enumerate(users.tolist()):
            hh, rr, tt = (x[u, hop].tolist() for x in (h, r, t))
            s = np.array([Un[b, rr[i]] @ E[hh[i]] for i in range(M)])
            pb = np.exp(s - s.max()) / np.exp(s - s.max()).sum()
            assert np.abs(pb - p[b].detach().numpy()).max() < 1e-14
            gp = np.array([E[tt[i]] @ c[b].numpy() for i in range(M)])
            gl = pb * (gp - (pb * gp).sum())
            for i in range(M):
                want_o[b] += pb[i] * E[tt[i]]
                want_ge[tt[i]] += pb[i] * c[b].numpy()
                want_ge[hh[i]] += gl[i] * Un[b, rr[i]]
                want_gU[b, rr[i]] += gl[i] * E[hh[i]]
        assert np.abs(o.detach().numpy() - want_o).max() < 1e-13
        assert np.abs(ge.numpy() - want_ge).max() < 1e-13 and np.abs(gU.numpy() - want_gU).max() < 1e-13
    with pytest.raises(ValueError):
        K.ripple_hop(ent, U, sets, users, 2)
    with pytest.raises(ValueError):
        K.ripple_hop(ent, U[:, :2], sets, users, 0)


# ------------------------------------------------------------------------------------------------ the model
def _toy_model(**kw):
    trip, pairs, _ = small_ckg()
    sets = K.RippleSets.build(trip, pairs, N_USERS, N_NODES, n_hop=2, n_memory=6, seed=2, add_inverse=True)
    torch.manual_seed(4)
    m = K.RippleNet(N_NODES, sets, dim=8, item_range=(5, 15), **kw).double()
    with torch.no_grad():
        m.entity_emb.weight.mul_(3.0)
    return m, sets


BATCH = (torch.tensor([0, 1, 4, 4, 3]), torch.tensor([5, 9, 10, 14, 24]), torch.tensor([8, 8, 23, 6, 7]))


@pytest.mark.parametrize("mode", ripple_models.UPDATE_MODES)
@pytest.mark.parametrize("all_hops", [True, False])
def test_ripplenet_forward_is_the_stated_model(mode, all_hops):
    m, sets = _toy_model(item_update_mode=mode, using_all_hops=all_hops)
    assert {k: tuple(v.shape) for k, v in m.named_parameters()} == {
        "entity_emb.weight": (N_NODES, 8), "relation_emb.weight": (sets.n_rel, 64), "transform_matrix.weight": (8, 8)}
    u, pos, _ = BATCH
    y = m.score(u, pos).detach()
    E, W = m.entity_emb.weight.detach(), m.transform_matrix.weight.detach()
    R = m.relation_emb.weight.detach().view(sets.n_rel, 8, 8)
    for b in range(u.numel()):
        v, os_ = E[pos[b]], []
        for k in range(2):
            h, r, t = (getattr(sets, n)[u[b], k].long() for n in ("mem_h", "mem_r", "mem_t"))
            s = torch.stack([v @ R[r[i]] @ E[h[i]] for i in range(6)])
            o = torch.softmax(s, 0) @ E[t]
            os_.append(o)
            v = {"replace": o, "plus": v + o, "replace_transform": o @ W.T, "plus_transform": (v + o) @ W.T}[mode]
        want = v @ (os_[0] + os_[1] if all_hops else os_[1])
        assert abs(float(y[b]) - float(want)) <= 1e-12 * max(1.0, abs(float(want))), (b, float(y[b]), float(want))
    loss = m.get_loss(*BATCH)
    loss.backward()
    grads = {k: v.grad for k, v in m.named_parameters()}
    assert grads["entity_emb.weight"].abs().sum() > 0 and grads["relation_emb.weight"].abs().sum() > 0
    assert grads["transform_matrix.weight"].abs().sum() > 0            # (the L2 term reaches W in every mode)
    assert all(torch.isfinite(g_).all() for g_ in grads.values())


def test_ripplenet_loss_terms():
    m, sets = _toy_model(kge_weight=0.25, reg_lambda=0.5)
    u, pos, neg = BATCH
    full = float(m.get_loss(u, pos, neg).detach())
    kge = float(m.kge_term(u).detach())
    m.kge_weight = 0.0
    bare = float(m.get_loss(u, pos, neg).detach())
    assert abs((full - bare) - 0.25 * kge) <= 1e-14 * max(1.0, abs(full))
    # the KGE term by hand: every hop triple of the batch's DISTINCT users
    E = m.entity_emb.weight.detach()
    R = m.relation_emb.weight.detach().view(sets.n_rel, 8, 8)
    vals = []
    for user in sorted(set(u.tolist())):
        for k in range(2):
            for i in range(6):
                h, r, t = (int(getattr(sets, n)[user, k, i]) for n in ("mem_h", "mem_r", "mem_t"))
                vals.append(torch.sigmoid(E[h] @ R[r] @ E[t]))
    assert abs(kge + float(torch.stack(vals).mean())) <= 1e-13
    # the rest: BCE over positives then negatives, and the L2 of the item rows, each o_k, R and W
    items = torch.cat([pos, neg])
    v, o_list = m.hops(torch.cat([u, u]), items)
    y = (v * (o_list[0] + o_list[1])).sum(1)
    y = y.detach()
    bce = torch.nn.functional.softplus(-y[:5]).sum() + torch.nn.functional.softplus(y[5:]).sum()
    half_sq = lambda x: float((x.detach() ** 2).sum(1).mean() / 2)   # noqa: E731
    l2 = half_sq(E[items]) + half_sq(o_list[0]) + half_sq(o_list[1]) + half_sq(m.relation_emb.weight) + half_sq(m.transform_matrix.weight)
    assert abs(bare - (float(bce) / 10 + 0.5 * l2)) <= 1e-13 * max(1.0, abs(bare))


@pytest.mark.parametrize("mode", ripple_models.UPDATE_MODES)
def test_ripplenet_scores_equal_per_pair_evaluation(mode):
    """The all-pairs factorisation against the per-pair path, in fp32: both sum d and M terms per score."""
    m, sets = _toy_model(item_update_mode=mode)
    m = m.float()
    users = torch.tensor([0, 3, 4, 3, 2])                              # a repeated user, and the invalid one
    sc = m.scores(users, max_bytes=2048)                              # several user blocks
    uu, ii = torch.meshgrid(users, torch.arange(5, 15), indexing="ij")
    y = m.score(uu.reshape(-1), ii.reshape(-1)).detach().reshape(5, 10)
    y64 = m.double().score(uu.reshape(-1), ii.reshape(-1)).detach().reshape(5, 10)
    assert sc.shape == y.shape == (5, 10)
    bar = 64 * 2.0 ** -24 * float(y64.abs().max())
    assert float((sc.double() - y64).abs().max()) <= bar and float((y.double() - y64).abs().max()) <= bar
    assert m.n_items == 10 and tuple(m.scores(users[:0]).shape) == (0, 10)


def test_ripplenet_loads_the_release_names_and_is_exported():
    m, sets = _toy_model()
    sd = {"entity_emb.weight": torch.randn(N_NODES, 8), "relation_emb.weight": torch.randn(sets.n_rel, 64),
          "transform_matrix.weight": torch.randn(8, 8)}
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.transform_matrix.weight.float(), sd["transform_matrix.weight"])
    assert K.ripple_models.RippleNet is K.RippleNet and K.ripple_models.RippleSets is K.RippleSets
    assert K.ripple_hop is autograd.ripple_hop and all(n in K.__all__ for n in ("RippleSets", "RippleNet", "ripple_hop"))
    with pytest.raises(ValueError):
        K.RippleNet(N_NODES, sets, item_update_mode="minus")
    with pytest.raises(ValueError):
        K.RippleNet(N_NODES + 1, sets)


# ------------------------------------------------------------------------------------------------ the entries
NEW = {"kgat_ripple_supported", "kgat_ripple_hop_fwd_f32", "kgat_ripple_hop_bwd_f32"}
ENTRIES = {"kgat_ripple_hop_fwd_f32": "ripple_hop_fwd", "kgat_ripple_hop_bwd_f32": "ripple_hop_bwd"}
_SIZES = dict(n_samples=2048, d=64, n_memory=32, n_rel=39, n_hop=2, hop=1, n_nodes=5000, n_users=900)


def call_entry(entry, sizes=None, pointers=None):
    """The entry with non-null, aligned host addresses it never gets as far as using: (return code, message)."""
    lib = _lib.load()
    s = dict(_SIZES, **(sizes or {}))
    args = []
    for ctype, pname in declarations()[entry][1]:
        if pname == "stream":
            args.append(None)
        elif pointers and pname in pointers:
            args.append(pointers[pname])
        elif "*" in ctype:
            args.append(P)
        else:
            args.append(s[pname])
    rc = getattr(lib, entry)(*args)
    return rc, (lib.kgat_last_error() or b"").decode()


def test_new_symbols_are_declared_exported_and_bound():
    decl = declarations()
    assert {n for n in decl if n.startswith("kgat_ripple")} == NEW
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        ret, params = decl[name]
        assert len(params) == len(_lib.SIGNATURES[name][1])
        # the closed tables of the workspace and memory-contract tests do not see these names
        assert not name.endswith("_workspace_bytes")
        assert not any(p == "workspace" or (t == "float *" and (p == "tmp" or p.startswith(("partials", "part_")))) for t, p in params)
    assert "kgat_ripple.hip" in _lib.SOURCES and _lib.ABI_VERSION == 16 and lib.kgat_version() == 16
    text = open(os.path.join(ROOT, "dgl-kgat_amd", "ops.py")).read()
    body = text.split("# ---------------------------------------------------------------- ripple-set attention")[1].split("# ------------------")[0]
    assert ".new_" not in body and "kgat_ripple_hop_bwd_f32" in body and "csr_from_coo(" in body and "spmm(" in body


def test_supported_is_the_envelope():
    lib = _lib.load()
    ok = lambda d, m=32, r=39, n=2048: bool(lib.kgat_ripple_supported(d, m, r, n))   # noqa: E731
    assert all(ok(d) for d in (16, 32, 64, 128)) and ok(64, 1) and ok(64, 128) and ok(64, 32, 1) and ok(64, 32, 4096) and ok(64, 32, 39, 1)
    assert not any(ok(d) for d in (0, 4, 8, 24, 48, 96, 256, -16))
    assert not ok(64, 0) and not ok(64, 129) and not ok(64, 32, 0) and not ok(64, 32, 4097) and not ok(64, 32, 39, 0)
    assert ok(64, 32, 39, 4 * (2 ** 31 - 1)) and not ok(64, 32, 39, 4 * (2 ** 31 - 1) + 1)
    from dgl_kgat_amd import ops
    assert ops.ripple_supported(16, 32, 39, 20480) and not ops.ripple_supported(20, 32, 39, 20480)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_refusals_come_before_device_work(entry):
    word = ENTRIES[entry]
    for sizes in (dict(d=0), dict(d=20), dict(d=256), dict(n_memory=0), dict(n_memory=129), dict(n_rel=0), dict(n_rel=4097),
                  dict(n_samples=0)):
        rc, msg = call_entry(entry, sizes)
        assert rc == UNSUPPORTED and word in msg, (sizes, rc, msg)
    for sizes in (dict(n_samples=-1), dict(d=-64), dict(n_memory=-1), dict(n_rel=-1), dict(n_nodes=0), dict(n_nodes=2 ** 31 - 1),
                  dict(n_users=0), dict(n_users=-2), dict(n_hop=0), dict(hop=-1), dict(hop=2), dict(n_hop=1, hop=1)):
        rc, msg = call_entry(entry, sizes)
        assert rc == BADARG and word in msg, (sizes, rc, msg)
    aligned = {"kgat_ripple_hop_fwd_f32": ("ent", "U", "o"), "kgat_ripple_hop_bwd_f32": ("ent", "U", "g_o", "grad_U")}[entry]
    for ctype, pname in declarations()[entry][1]:
        if "*" in ctype:
            rc, msg = call_entry(entry, pointers={pname: None})
            assert rc == BADARG and word in msg and "null" in msg, (pname, rc, msg)
            rc, msg = call_entry(entry, pointers={pname: P + 4})
            if pname in aligned:
                assert rc == BADARG and word in msg and "aligned" in msg, (pname, rc, msg)
    assert OK == 0


def test_cpu_tensors_are_refused_by_the_raw_wrappers():
    from dgl_kgat_amd import ops
    z = np.zeros((2, 1, 3), dtype=np.int64)
    sets = K.RippleSets(z, z, z, 4, 2)
    with pytest.raises(K.KGATLibraryError):
        ops.ripple_hop_fwd(torch.zeros(4, 16), torch.zeros(1, 2, 16), sets, torch.zeros(1, dtype=torch.int32), 0)


# ------------------------------------------------------------------------------------------------ the harness
def test_cli_accepts_and_refuses():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_kgat
    base = vars(train_kgat.parse_args([]))
    assert not any(f in base for f in train_kgat.RIPPLE_FLAGS)          # a run without the flags keeps its arguments
    a = train_kgat.parse_args(["--model", "ripplenet", "--n_hop", "3", "--n_memory", "16", "--kge_weight", "0", "--item_update_mode",
                               "plus", "--using_all_hops", "0", "--ripple_inverse", "1", "--Ks", "20,40", "--grad_norm", "1.0",
                               "--eval_before", "--log_json", "x.json"])
    assert (a.model, a.n_hop, a.n_memory, a.kge_weight, a.item_update_mode, a.using_all_hops, a.ripple_inverse) == \
        ("ripplenet", 3, 16, 0.0, "plus", 0, 1)
    for flags in (["--rank_metrics", "1"], ["--gpus", "2"], ["--explain", "3"], ["--n_hop", "0"], ["--n_hop", "5"], ["--n_memory", "129"],
                  ["--n_memory", "0"], ["--item_update_mode", "minus"], ["--using_all_hops", "2"], ["--ripple_inverse", "2"],
                  ["--kg_eval", "50"], ["--gnn_model", "rgcn"], ["--pretrain_epochs", "1"], ["--nfm_layers", "32"]):
        with pytest.raises(SystemExit) as e:
            train_kgat.parse_args(["--model", "ripplenet"] + flags)
        assert e.value.code == 2, flags
    for flags in (["--n_hop", "2"], ["--model", "fm", "--n_memory", "32"], ["--model", "cke", "--kge_weight", "0.1"],
                  ["--ripple_inverse", "1"], ["--model", "nfm", "--item_update_mode", "plus"], ["--using_all_hops", "1"]):
        with pytest.raises(SystemExit) as e:
            train_kgat.parse_args(flags)
        assert e.value.code == 2, flags
