"""TransE / CFKG / CKE without a GPU: the float64 restatement against the reference-validated TransR restatement with
identity projections, the models' parameters and state, the readout's ordering, every new entry's refusals (made before
any device work: they come back on a machine without a device), link prediction on the torch route, and the harness's
refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import dgl_kgat_amd as K  # noqa: E402
from dgl_kgat_amd import _lib  # noqa: E402

import _kg_rank_ref as KR  # noqa: E402
import _transe_ref as T  # noqa: E402
from test_workspace_host import BADARG, OK, P, WORKSPACE, declarations  # noqa: E402

UNSUPPORTED = -2


# ------------------------------------------------------------------------------------------------ the objective
@pytest.mark.parametrize("name", ["20-xavier-N700-R9-B1200", "64-zeros-N700-R9-B1200", "8-xavier-N700-R9-B3"])
def test_restatement_is_transr_with_identity_projections(name):
    """The float64 restatement (loss and both gradients) against KGATPropagation.transR(fused=False) with every
    W_R[r] = I and d = k, in float64: equal to rounding - the constant regulariser term included."""
    c = next(c for c in T.TRANSE_CASES if c.name == name)
    (h, r, pt, nt), (ent, rel), ref, _ = T.transe_case_data(name)
    m = K.KGATPropagation(c.N, c.R, c.d, c.d, 1, 16, 0.0).double()
    with torch.no_grad():
        m.entity_embed.weight.copy_(ent)
        m.relation_embed.weight.copy_(rel)
        m.W_R.copy_(torch.eye(c.d, dtype=torch.float64).expand(c.R, c.d, c.d))
    ids = [torch.as_tensor(x) for x in (h, r, pt, nt)]
    loss = m.transR(*ids, T.REG_LAMBDA, fused=False)
    loss.backward()
    assert abs(float(loss.detach()) - ref.loss) <= 1e-13 * abs(ref.loss)
    for got, want in ((m.entity_embed.weight.grad, ref.grad_ent), (m.relation_embed.weight.grad, ref.grad_rel)):
        got = got.numpy()
        assert np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300)
    # and the model's own torch route states the same objective
    cf = K.CFKG(c.N, c.R, dim=c.d, reg_lambda_kg=T.REG_LAMBDA).double()
    with torch.no_grad():
        cf.entity_embed.weight.copy_(ent)
        cf.relation_embed.weight.copy_(rel)
    assert abs(float(cf.transE(*ids).detach()) - ref.loss) <= 1e-13 * abs(ref.loss)


def test_fp32_restatement_clears_every_bar():
    """The CPU fp32 restatement against the bars the device is held to (a bar the comparator itself misses would be no bar)."""
    for c in T.TRANSE_CASES:
        if c.N > 1000:
            continue
        _, _, ref, rs = T.transe_case_data(c.name)
        err = T.transe_errors(ref, (rs.grad_ent, rs.grad_rel))
        assert all(np.isfinite(e).all() for e in err), c.name
        assert all(T.bar_ratio(e, e, f) <= 1.0 for e, f in zip(err, T.transe_floors(ref, c.d))), c.name
        assert T.loss_ok(rs.loss, rs.loss, ref.loss)


# ------------------------------------------------------------------------------------------------ the models
def test_parameters_and_state_dict_round_trip():
    cf = K.CFKG(50, 5, dim=8)
    assert {k: tuple(v.shape) for k, v in cf.named_parameters()} == {"entity_embed.weight": (50, 8), "relation_embed.weight": (5, 8)}
    ck = K.CKE(50, 5, dim=8, relation_dim=12, reg_lambda_kg=0.02, reg_lambda_cf=0.03)
    assert {k: tuple(v.shape) for k, v in ck.named_parameters()} == {
        "entity_embed.weight": (50, 8), "relation_embed.weight": (5, 12), "W_R": (5, 8, 12), "cf_embed.weight": (50, 8)}
    assert not hasattr(cf, "W_R")
    for make, m in ((lambda: K.CFKG(50, 5, dim=8), cf), (lambda: K.CKE(50, 5, dim=8, relation_dim=12), ck)):
        other = make()
        other.load_state_dict(m.state_dict())
        assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), other.state_dict().values()))
    assert K.kge_models.CFKG is K.CFKG and K.kge_models.CKE is K.CKE


def test_cke_is_composition_over_the_transr_and_bpr_code():
    """CKE's TransR part is KGATPropagation's own functions; its BPR gradient reaches cf_embed and the ITEM rows of
    entity_embed only."""
    ck = K.CKE(40, 3, dim=8, relation_dim=8)
    for name in ("transR", "kg_step", "kg_phase", "get_loss"):
        assert getattr(K.CKE, name) is getattr(K.KGATPropagation, name), name
    items = (10, 30)
    ro = ck.readout(items)
    assert torch.equal(ro[:10], ck.cf_embed.weight[:10]) and torch.equal(ro[30:], ck.cf_embed.weight[30:])
    assert torch.equal(ro[10:30], ck.cf_embed.weight[10:30] + ck.entity_embed.weight[10:30])
    g = torch.Generator().manual_seed(0)
    u, p, n = torch.randint(0, 10, (16,), generator=g), torch.randint(10, 30, (16,), generator=g), torch.randint(10, 30, (16,), generator=g)
    ck.get_loss(ro, u, p, n).backward()
    ge = ck.entity_embed.weight.grad
    assert ck.cf_embed.weight.grad.abs().sum() > 0 and ge[10:30].abs().sum() > 0 and not ge[:10].any() and not ge[30:].any()
    assert ck.W_R.grad is None
    opt = torch.optim.Adam(ck.parameters(), lr=0.01)
    h, r, t, q = (torch.randint(0, hi, (2, 6), generator=g) for hi in (40, 3, 40, 40))
    losses = ck.kg_phase(h, r, t, q, opt)
    assert losses.shape == (2,) and torch.isfinite(losses).all()


def test_cfkg_grad_is_none_after_every_cpu_route():
    cf = K.CFKG(40, 3, dim=8)
    g = torch.Generator().manual_seed(1)
    h, r, t, q = (torch.randint(0, hi, (3, 6), generator=g) for hi in (40, 3, 40, 40))
    opt = torch.optim.Adam(cf.parameters(), lr=0.01)
    before = cf.entity_embed.weight.detach().clone()
    cf.entity_embed.weight.grad = torch.ones_like(before)
    losses = cf.kg_phase(h, r, t, q, opt)
    assert losses.shape == (3,) and not torch.equal(before, cf.entity_embed.weight)
    assert cf.entity_embed.weight.grad is None and cf.relation_embed.weight.grad is None
    cf.kg_step(h[0], r[0], t[0], q[0], opt)
    assert cf.entity_embed.weight.grad is None and cf.relation_embed.weight.grad is None
    assert cf.kg_phase(h[:0], r[:0], t[:0], q[:0], opt).shape == (0,)


def test_readout_orders_items_as_the_distance_does():
    """Dyadic unit rows (sixteen elements of +-1/4), so that float64 holds every q . i and |q - i|^2 exactly: the
    order by descending q . i equals the order by ascending |q - i|^2, ties broken by id in both."""
    rng = np.random.default_rng(3)
    n_users, n_items, n_attr, d = 12, 60, 8, 32
    N = n_users + n_items + n_attr

    def unit(n):
        x = np.zeros((n, d))
        for i in range(n):
            x[i, rng.choice(d, 16, replace=False)] = rng.choice([-0.25, 0.25], 16)
        return x
    ent, rel = unit(N), unit(3)
    ent[n_users + 7] = ent[n_users + 3]                            # two items tie for every user
    cf = K.CFKG(N, 3, dim=d).double()
    with torch.no_grad():
        cf.entity_embed.weight.copy_(torch.as_tensor(ent) * 3.0)   # any positive scale: the readout normalises
        cf.relation_embed.weight.copy_(torch.as_tensor(rel) * 0.5)
    table = cf.readout(2, (0, n_users), (n_users, n_users + n_items)).detach().numpy()
    assert np.array_equal(table[n_users:], ent[n_users:]) and np.array_equal(table[:n_users], ent[:n_users] + rel[2])
    q, it = table[:n_users], table[n_users:n_users + n_items]
    dot = q @ it.T
    dist = ((q[:, None, :] - it[None, :, :]) ** 2).sum(2)
    ids = np.arange(n_items)
    for u in range(n_users):
        by_dot = np.lexsort((ids, -dot[u]))
        by_dist = np.lexsort((ids, dist[u]))
        assert np.array_equal(by_dot, by_dist), u
        assert list(by_dot).index(3) < list(by_dot).index(7) and dot[u, 3] == dot[u, 7]   # the tie, lower id first
    with pytest.raises(ValueError):
        cf.readout(2, (0, 20), (10, 40))
    with pytest.raises(IndexError):
        cf.readout(3, (0, n_users), (n_users, n_users + n_items))


# ------------------------------------------------------------------------------------------------ the entries' refusals
_SIZES = dict(n_nodes=1000, n_rel=41, d=64, batch=65, n_batches=2, reg_lambda=0.01, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
              tag=1)
_MOMENTS = (C.c_void_p * 2)(P, P)
_STEPS = (C.c_int64 * 2)(1, 1)
_HOST = dict(exp_avg_host=C.addressof(_MOMENTS), exp_avg_sq_host=C.addressof(_MOMENTS), steps_host=C.addressof(_STEPS))
# entry -> the word kgat_last_error must carry
ENTRIES = {"kgat_transe_forward_f32": "transe_forward", "kgat_transe_backward_f32": "transe_backward",
           "kgat_transe_loss_grad_f32": "transe_loss_grad", "kgat_transe_presort_f32": "transe_presort",
           "kgat_transe_adam_step_f32": "transe_adam_step"}


def _call(entry, sizes=None, pointers=None, short=0):
    lib = _lib.load()
    s = dict(_SIZES, **(sizes or {}))
    ptrs = dict(_HOST, **(pointers or {}))
    args = []
    for ctype, pname in declarations()[entry][1]:
        if pname == "scratch_bytes":
            args.append(lib.kgat_transe_scratch_bytes(s["batch"], s["d"], s["n_rel"]) - short)
        elif pname == "sorted_bytes":
            args.append(s["n_batches"] * lib.kgat_transe_sorted_bytes(s["batch"], s["n_rel"]) - short)
        elif pname == "stream":
            args.append(None)
        elif pname in ptrs:
            args.append(ptrs[pname])
        elif "*" in ctype:
            args.append(P)
        else:
            args.append(s[pname])
    rc = getattr(lib, entry)(*args)
    return rc, (lib.kgat_last_error() or b"").decode()


def test_every_new_entry_is_in_the_table():
    new = {n for n in declarations() if n.startswith("kgat_transe_")}
    assert new == set(ENTRIES) | {"kgat_transe_supported", "kgat_transe_scratch_bytes", "kgat_transe_sorted_bytes"}
    for name, (_, params) in declarations().items():
        if name in new:     # the closed tables of the workspace and memory-contract tests do not see these names
            assert not name.endswith("_workspace_bytes")
            assert not any(p == "workspace" or (t == "float *" and (p == "tmp" or p.startswith(("partials", "part_")))) for t, p in params)


def test_supported_is_the_envelope():
    lib = _lib.load()
    ok = lambda n, d, r, b: bool(lib.kgat_transe_supported(n, d, r, b))   # noqa: E731
    assert all(ok(1000, d, 41, 2048) for d in (4, 8, 20, 64, 128, 256))
    assert not any(ok(1000, d, 41, 2048) for d in (0, 2, 6, 260, -4))
    assert ok(1, 4, 1, 1) and ok(2 ** 31 - 2, 64, 4096, 2730)
    assert not ok(1000, 64, 41, 2731) and not ok(1000, 64, 41, 0) and not ok(1000, 64, 4097, 10) and not ok(1000, 64, 0, 10)
    assert not ok(0, 64, 41, 10) and not ok(2 ** 31 - 1, 64, 41, 10)
    assert lib.kgat_transe_sorted_bytes(65, 41) == lib.kgat_transr_sorted_bytes(65, 41) > 0
    assert lib.kgat_transe_scratch_bytes(65, 64, 41) > lib.kgat_transe_sorted_bytes(65, 41) + 4 * 65 * 64 * 4


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_refusals_come_before_device_work(entry):
    word = ENTRIES[entry]
    params = declarations()[entry][1]
    # one byte short of the stated size
    rc, msg = _call(entry, short=1)
    assert rc == WORKSPACE and word in msg, (rc, msg)
    # sizes outside kgat_transe_supported
    bad = [dict(batch=2731), dict(batch=0), dict(batch=-1), dict(n_rel=4097), dict(n_rel=0), dict(n_nodes=0), dict(n_nodes=-5),
           dict(n_nodes=2 ** 31 - 1)]
    if entry != "kgat_transe_presort_f32":
        bad += [dict(d=6), dict(d=0), dict(d=-4), dict(d=260)]
    for sizes in bad:
        rc, msg = _call(entry, sizes)
        assert rc == UNSUPPORTED and word in msg, (sizes, rc, msg)
    # a null pointer, one parameter at a time (grad_scale may be NULL)
    for ctype, pname in params:
        if "*" in ctype and pname != "grad_scale":
            rc, msg = _call(entry, pointers={pname: None})
            assert rc == BADARG and word in msg, (pname, rc, msg)
    # a misaligned buffer
    target = "sorted" if entry == "kgat_transe_presort_f32" else "scratch"
    rc, msg = _call(entry, pointers={target: P + 4})
    assert rc == BADARG and word in msg, (rc, msg)
    if entry == "kgat_transe_presort_f32":
        rc, msg = _call(entry, dict(n_batches=-1))
        assert rc == BADARG and word in msg
        assert _call(entry, dict(n_batches=0))[0] == OK           # nothing to sort: no device work
    if entry == "kgat_transe_adam_step_f32":
        for sizes in (dict(tag=0), dict(tag=1 << 50), dict(lr=-1.0), dict(beta1=1.0), dict(beta2=-0.1), dict(eps=-1e-8)):
            rc, msg = _call(entry, sizes)
            assert rc == BADARG and word in msg, (sizes, rc, msg)
        zero_steps = (C.c_int64 * 2)(1, 0)
        rc, msg = _call(entry, pointers=dict(steps_host=C.addressof(zero_steps)))
        assert rc == BADARG and word in msg


def test_ops_wrappers_allocate_through_the_module_helpers():
    text = open(os.path.join(ROOT, "dgl-kgat_amd", "ops.py")).read()
    body = text.split("# ---------------------------------------------------------------- TransE KG embedding")[1].split("# ------------------")[0]
    assert ".new_empty(" not in body and ".new_zeros(" not in body and "kgat_transe_adam_step_f32" in body
    assert "kgat_transe.hip" in _lib.SOURCES


# ------------------------------------------------------------------------------------------------ link prediction
@pytest.mark.parametrize("side", ["tail", "head"])
def test_kg_rank_without_projection_agrees_with_a_literal_loop(side):
    """A model without W_R on the CPU takes the torch route: the counts of a literal float64 loop (one triple and one
    candidate at a time, u = x / max(|x|, 1e-12), no projection), filtered, on a candidate range."""
    g = torch.Generator().manual_seed(5)
    N, n_rel, d = 40, 3, 8
    cf = K.CFKG(N, n_rel, dim=d).double()
    with torch.no_grad():
        cf.entity_embed.weight.copy_(torch.randn(N, d, generator=g, dtype=torch.float64))
        cf.entity_embed.weight[4] = 0.0
        cf.relation_embed.weight.copy_(torch.randn(n_rel, d, generator=g, dtype=torch.float64))
    rng = np.random.default_rng(6)
    lo, hi = 5, 35
    trip = np.stack([rng.integers(lo, hi, 25), rng.integers(0, n_rel, 25), rng.integers(lo, hi, 25)], 1)
    extra = np.stack([rng.integers(0, N, 80), rng.integers(0, n_rel, 80), rng.integers(0, N, 80)], 1)
    allt = np.concatenate([trip, extra])
    known = K.KnownTriples(allt[:, 0], allt[:, 1], allt[:, 2], N, n_rel)
    got = cf.kg_rank(trip[:, 0], trip[:, 1], trip[:, 2], known=known, side=side, candidates=(lo, hi))
    eye = np.broadcast_to(np.eye(d), (n_rel, d, d))
    lt, eq = KR.loop_counts(cf.entity_embed.weight.detach().numpy(), eye, cf.relation_embed.weight.detach().numpy(),
                            [tuple(x) for x in trip], {tuple(x) for x in allt}, side, lo, hi)
    # (the loop scores in the direct form, kg_rank by n2 - 2 q.p: the same order away from ties of rounding size)
    assert np.abs(got.lt.numpy() - np.asarray(lt)).max() <= 0 and np.array_equal(got.eq.numpy(), np.asarray(eq))
    m = cf.kg_metrics(trip[:, 0], trip[:, 1], trip[:, 2], known=known, side=side, hits=(1, 10))
    assert m["n"] == 25 and 0 < m["mrr"] <= 1


def test_kg_rank_of_a_model_with_projection_is_untouched():
    """kg_eval's branch is taken only without W_R: a KGATPropagation ranks through the same code as before."""
    m = KR.make_model(K, 300, 16, 16, "cpu")
    q = KR.e2e_queries(300, 16, 16, "tail", False, False)
    case = KR.e2e_case(300, 16, 16, "tail", False, False)
    got = m.kg_rank(q[:, 0], q[:, 1], q[:, 2], known=None, side="tail")
    assert (got.lt.numpy() >= case.lt_lo).all()                    # unfiltered counts can only exceed the filtered band's floor


# ------------------------------------------------------------------------------------------------ the harness
def test_cli_refusals_and_the_default_run_keeps_its_arguments():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_kgat
    base = vars(train_kgat.parse_args([]))
    assert "model" not in base and "num_bases" not in base        # a run without the flag: the --log_json args of before
    assert train_kgat.parse_args(["--model", "cfkg", "--kg_eval", "50", "--Ks", "20,40", "--rank_metrics", "1"]).model == "cfkg"
    assert train_kgat.parse_args(["--model", "cke", "--pretrain_load", "mf.npz"]).pretrain_load == "mf.npz"
    for model in ("cfkg", "cke"):
        for flags in (["--gnn_model", "graphsage"], ["--gnn_model", "rgcn"], ["--res_type", "GCN"], ["--node_dropout", "0.1"],
                      ["--attention_grad", "1"], ["--explain", "3"], ["--use_attention", "0"], ["--gpus", "2"],
                      ["--num_bases", "2"], ["--pretrain_epochs", "1"], ["--pretrain_save", "mf.npz"]):
            with pytest.raises(SystemExit) as e:
                train_kgat.parse_args(["--model", model] + flags)
            assert e.value.code == 2, (model, flags)
    with pytest.raises(SystemExit):
        train_kgat.parse_args(["--model", "transe"])
