"""BPR-MF pretraining, the host side (no GPU): the ABI, the argument refusals of kgat_mf_*, mf_step / mf_phase on a CPU
module against the hand-written loop, the mf.npz format, and the harness flags."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("kgat_mf_supported", "kgat_mf_sorted_bytes", "kgat_mf_presort_f32", "kgat_mf_step_workspace_bytes",
               "kgat_mf_adam_step_f32")
BADARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
_BUF = C.create_string_buffer(4096 + 16)   # a non-null, 16-byte aligned address; no case below gets as far as reading it
P = (C.addressof(_BUF) + 15) // 16 * 16


def _lib():
    from dgl_kgat_amd import _lib
    return _lib


def al(x):
    return (x + 255) // 256 * 256


def test_header_declares_the_entries_at_abi_16_and_the_library_exports_them():
    lib = _lib()
    with open(lib.HEADER) as fh:
        text = fh.read()
    assert re.search(r"#define\s+KGAT_ABI_VERSION\s+16\b", text)
    assert lib.ABI_VERSION == 16
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in lib.SIGNATURES, name
    # the entry's documentation names what it restates
    doc = text[text.index("BPR-MF pretraining"):text.index("int kgat_mf_supported")]
    assert "models.py:170-178" in doc and "kgat.py:150-168" in doc and "row_slot" in doc
    assert lib.load().kgat_version() == 16
    so = C.CDLL(lib.SO_PATH)       # (symbol lookup only: nothing is called)
    for name in NEW_SYMBOLS:
        assert hasattr(so, name), name


def test_return_codes_are_the_headers():
    with open(_lib().HEADER) as fh:
        text = fh.read()
    for name, val in (("KGAT_E_BADARG", BADARG), ("KGAT_E_UNSUPPORTED", UNSUPPORTED), ("KGAT_E_WORKSPACE", WORKSPACE)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, val), text), name


def test_supported_sizes():
    from dgl_kgat_amd import ops
    assert ops.mf_supported(159251, 64, 1024)
    # 2,730 is the last batch one workgroup sorts (3 * 2730 = 8190 <= 8192 < 8193); beyond it the slice sort + rank merge,
    # up to 65,536 ids: the reference's CF batch of 10,240 is inside, 21,845 the last
    assert ops.mf_supported(1000, 64, 2730) and ops.mf_supported(1000, 64, 2731) and ops.mf_supported(1000, 64, 10240)
    assert ops.mf_supported(1000, 64, 21845) and not ops.mf_supported(1000, 64, 21846)
    for F, want in ((4, True), (8, True), (16, True), (48, True), (256, True), (260, False), (6, False), (0, False), (-4, False)):
        assert ops.mf_supported(1000, F, 512) == want, F
    assert ops.mf_supported((1 << 31) - 2, 64, 16) and not ops.mf_supported((1 << 31) - 1, 64, 16)
    assert not ops.mf_supported(0, 64, 16) and not ops.mf_supported(-5, 64, 16) and not ops.mf_supported(1000, 64, 0)
    assert not ops.mf_supported(1000, 64, -3)


def test_size_entries():
    lib = _lib().load()
    for b in (1, 13, 64, 1024, 2730, 2731, 10240, 21845):
        scratch = al(8 * 3 * b) if 3 * b > 8192 else 0                      # the slice sort's packed lists
        assert lib.kgat_mf_sorted_bytes(b) == 3 * al(4 * 3 * b) + scratch, b   # sorted ids | order | run lengths
        for F in (4, 48, 64, 256):
            windows = -(-3 * b // 32)
            want = al(4 * 4 * b) + al(4 * b) + al(4 * 3 * b * F) + al(4 * windows * 2 * F)   # part | coef | compact | window partials
            assert lib.kgat_mf_step_workspace_bytes(b, F) == want, (b, F)


def _call(name, args):
    lib = _lib().load()
    rc = getattr(lib, name)(*args)
    return rc, (lib.kgat_last_error() or b"").decode()


def test_presort_refusals():
    lib = _lib().load()
    n, b, nb = 1000, 64, 3
    need = nb * lib.kgat_mf_sorted_bytes(b)
    ok = [n, nb, b, P, P, P, P, need, None]

    def with_(i, v):
        a = list(ok)
        a[i] = v
        return a
    for args, rc, frag in ((with_(1, -1), BADARG, "bad batch count"), (with_(2, 21846), UNSUPPORTED, "batch"),
                           ([n, 65536, 2731, P, P, P, P, 1 << 40, None], BADARG, "65,535 batches"),
                           (with_(2, 0), UNSUPPORTED, "batch"), (with_(2, -7), UNSUPPORTED, "batch"),
                           (with_(0, 0), UNSUPPORTED, "n_nodes"), (with_(0, -1), UNSUPPORTED, "n_nodes"),
                           (with_(0, 1 << 31), UNSUPPORTED, "n_nodes"),
                           (with_(3, None), BADARG, "null pointer"), (with_(4, None), BADARG, "null pointer"),
                           (with_(5, None), BADARG, "null pointer"), (with_(6, None), BADARG, "null pointer"),
                           (with_(7, need - 1), WORKSPACE, "output buffer too small")):
        got, msg = _call("kgat_mf_presort_f32", args)
        assert got == rc and frag in msg, (args, got, msg)
    assert _call("kgat_mf_presort_f32", with_(1, 0))[0] == 0    # no batches: nothing to do


def test_adam_step_refusals():
    lib = _lib().load()
    n, F, b = 1000, 64, 65
    need = lib.kgat_mf_step_workspace_bytes(b, F)
    #      0  1  2  3  4  5  6  7  8  9  10  11    12   13     14    15    16 17 18 19  20   21
    ok = [n, F, b, P, P, P, P, P, P, P, 1, 1e-3, 0.9, 0.999, 1e-8, 1e-5, P, P, 1, P, need, None]

    def with_(i, v):
        a = list(ok)
        a[i] = v
        return a
    cases = [(with_(1, 6), UNSUPPORTED, "multiple of 4"), (with_(1, 260), UNSUPPORTED, "multiple of 4"),
             (with_(1, -4), UNSUPPORTED, "multiple of 4"), (with_(2, 21846), UNSUPPORTED, "batch"),
             (with_(2, -1), UNSUPPORTED, "batch"), (with_(0, 0), UNSUPPORTED, "n_nodes"), (with_(0, -9), UNSUPPORTED, "n_nodes"),
             (with_(10, 0), BADARG, "step count"), (with_(11, -1.0), BADARG, "hyperparameter"),
             (with_(12, 1.0), BADARG, "hyperparameter"), (with_(13, -0.1), BADARG, "hyperparameter"),
             (with_(14, -1e-8), BADARG, "hyperparameter"), (with_(18, 0), BADARG, "tag"), (with_(18, 1 << 50), BADARG, "tag"),
             (with_(7, P + 4), BADARG, "16-byte aligned"), (with_(8, P + 8), BADARG, "16-byte aligned"),
             (with_(20, need - 1), WORKSPACE, "workspace too small")]
    cases += [(with_(i, None), BADARG, "null pointer") for i in (3, 4, 5, 6, 7, 8, 9, 16, 17, 19)]
    for args, rc, frag in cases:
        got, msg = _call("kgat_mf_adam_step_f32", args)
        assert got == rc and frag in msg, (args, got, msg)


# ---- mf_step / mf_phase on a CPU module: the torch operators
def _cpu_model(n=60, d=8, seed=0, dtype=torch.float32):
    import dgl_kgat_amd as K
    torch.manual_seed(seed)
    return K.KGATPropagation(n, 3, d, d, 1, d, dropout=0.0, reg_lambda_gnn=1e-3).to(dtype)


def _ids(n, n_it, B, seed=5):
    g = torch.Generator().manual_seed(seed)
    u, p, q = (torch.randint(0, n, (n_it, B), generator=g) for _ in range(3))
    p[0, :4] = u[0, :4]
    p[1, 3:9] = 7
    return u, p, q


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_cpu_mf_phase_is_the_handwritten_loop(dtype):
    n, n_it, B = 60, 4, 11
    u, p, q = _ids(n, n_it, B)
    a, b = _cpu_model(dtype=dtype), _cpu_model(dtype=dtype)
    oa, ob = torch.optim.Adam(a.parameters(), lr=0.05), torch.optim.Adam(b.parameters(), lr=0.05)
    before = [t.detach().clone() for t in a.parameters()]
    got = a.mf_phase(u, p.int(), q, oa)           # (int32 and int64 ids are both taken)
    want = []
    for i in range(n_it):
        loss = b.get_loss(b.entity_embed.weight, u[i], p[i], q[i])
        loss.backward(); ob.step(); ob.zero_grad()
        want.append(loss.detach())
    assert got.shape == (n_it,) and got.dtype == dtype and torch.equal(got, torch.stack(want))
    ea, eb = a.entity_embed.weight, b.entity_embed.weight
    ent_before = next(t0 for t, t0 in zip(a.parameters(), before) if t is ea)
    assert torch.equal(ea, eb) and not torch.equal(ea, ent_before)
    sa, sb = oa.state[ea], ob.state[eb]
    assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])
    assert float(sa["step"]) == float(sb["step"]) == n_it
    # the other parameters: not updated, no optimiser state, no gradient
    for (name, t), t0 in zip(a.named_parameters(), before):
        if t is ea:
            continue
        assert torch.equal(t, t0) and t.grad is None and t not in oa.state, name
    assert ea.grad is None
    # a second phase goes on from the first's state; mf_step is one iteration of it
    more = a.mf_phase(u[:1], p[:1], q[:1], oa)
    one = b.mf_step(u[0], p[0], q[0], ob)
    assert torch.equal(more[0], one) and torch.equal(ea, eb) and float(oa.state[ea]["step"]) == n_it + 1


def test_cpu_mf_reg_lambda_and_edge_cases():
    n, n_it, B = 60, 3, 7
    u, p, q = _ids(n, n_it, B)
    a, b = _cpu_model(), _cpu_model()
    oa, ob = torch.optim.SGD(a.parameters(), lr=0.1), torch.optim.SGD(b.parameters(), lr=0.1)   # any torch optimiser
    got = a.mf_phase(u, p, q, oa, reg_lambda=0.5)
    b._reg_lambda_gnn = 0.5
    want = []
    for i in range(n_it):
        loss = b.get_loss(b.entity_embed.weight, u[i], p[i], q[i])
        loss.backward(); ob.step(); ob.zero_grad()
        want.append(loss.detach())
    assert torch.equal(got, torch.stack(want)) and torch.equal(a.entity_embed.weight, b.entity_embed.weight)
    assert a._reg_lambda_gnn == 1e-3                                  # the model's own regulariser is left as it was
    empty = a.mf_phase(u[:0], p[:0], q[:0], oa)
    assert empty.shape == (0,) and empty.dtype == torch.float32
    for bad in ((u, p[:2], q), (u, p, q[:, :3]), (u[0], p[0], q[0])):
        with pytest.raises(ValueError):
            a.mf_phase(*bad, oa)
    with pytest.raises(ValueError):
        a.mf_step(u[0], p[0][:3], q[0], oa)


# ---- mf.npz
def test_pretrain_file_round_trip(tmp_path):
    from dgl_kgat_amd import ckg_io
    rng = np.random.default_rng(0)
    ue, ie = rng.standard_normal((5, 8)).astype(np.float32), rng.standard_normal((9, 8)).astype(np.float32)
    ue[0, 0], ie[0, 0] = np.float32(-0.0), np.float32(1e-42)     # (a signed zero and a denormal keep their bits)
    path = str(tmp_path / "mf.npz")
    ckg_io.save_pretrain(path, ue, ie)
    with np.load(path) as z:
        assert sorted(z.files) == ["item_embed", "user_embed"] and z["user_embed"].dtype == np.float32
    gu, gi = ckg_io.load_pretrain(path)
    assert gu.dtype == gi.dtype == np.float32 and gu.tobytes() == ue.tobytes() and gi.tobytes() == ie.tobytes()
    # other keys are ignored; float64 arrays arrive as float32
    np.savez(path, user_embed=ue.astype(np.float64), item_embed=ie, extra=np.arange(3))
    gu, gi = ckg_io.load_pretrain(path)
    assert gu.dtype == np.float32 and np.array_equal(gu, ue) and np.array_equal(gi, ie)
    for bad in (dict(user_embed=ue), dict(item_embed=ie), dict(user_embed=ue, item_embed=ie[:, :4]),
                dict(user_embed=ue.reshape(-1), item_embed=ie), dict(user_embed=ue, item_embed=ie[None])):
        np.savez(path, **bad)
        with pytest.raises(ValueError):
            ckg_io.load_pretrain(path)
    with pytest.raises(ValueError):
        ckg_io.save_pretrain(path, ue, ie[:, :4])


def test_load_pretrained_writes_the_user_and_item_rows_only():
    from dgl_kgat_amd import ckg_io  # noqa: F401
    n_users, n_items, n = 5, 9, 20
    m = _cpu_model(n=n)
    before = m.entity_embed.weight.detach().clone()
    others = [t.detach().clone() for t in m.parameters()]
    rng = np.random.default_rng(1)
    ue, ie = rng.standard_normal((n_users, 8)).astype(np.float32), rng.standard_normal((n_items, 8)).astype(np.float32)
    m.load_pretrained(ue, ie, n_users)
    w = m.entity_embed.weight.detach()
    assert np.array_equal(w[:n_users].numpy(), ue) and np.array_equal(w[n_users:n_users + n_items].numpy(), ie)
    assert torch.equal(w[n_users + n_items:], before[n_users + n_items:])          # attribute entities: as they were
    for t, t0 in zip(m.parameters(), others):
        assert t is m.entity_embed.weight or torch.equal(t, t0)
    gu, gi = m.pretrained_embeddings(n_users, n_items)
    assert gu.dtype == np.float32 and gu.tobytes() == ue.tobytes() and gi.tobytes() == ie.tobytes()
    m.load_pretrained(torch.as_tensor(ue), torch.as_tensor(ie), n_users)            # tensors as well
    for bad in ((ue[:, :4], ie[:, :4], n_users), (ue, ie[:, :4], n_users), (ue, ie, n_users + 1), (ue[:3], ie, n_users),
                (ue, np.zeros((n - n_users + 1, 8), np.float32), n_users), (ue.reshape(-1), ie, n_users)):
        with pytest.raises(ValueError):
            m.load_pretrained(*bad)
    with pytest.raises(ValueError):
        m.pretrained_embeddings(n_users, n)


# ---- the harness
def _train_kgat():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_kgat
    return train_kgat


# every field of parse_args([]) at the parent commit
PARENT_DEFAULTS = dict(
    data_dir=None, synthetic=0.01, planted=False, epochs=2, entity_embed_dim=64, relation_embed_dim=64, gnn_num_layer=3,
    gnn_hidden_size=64, gnn_model="kgat", res_type="Bi", dropout_rate=0.1, use_attention=1, adj_type="si", node_dropout=0.0,
    attention_grad=0, lr=0.0001, grad_norm=0.0, batch_size=10240, batch_size_kg=2048, max_iters=0, seed=1234, gpus=1,
    eval_before=False, log_json=None, Ks=[20], grad_digest=False, explain=0, explain_top=1, kg_eval=0, kg_holdout=0.0)


def test_parser_flags(capsys):
    t = _train_kgat()
    a = vars(t.parse_args([]))
    for k, v in PARENT_DEFAULTS.items():
        assert a[k] == v, k
    new = {k: v for k, v in a.items() if k not in PARENT_DEFAULTS}
    assert new == dict(pretrain_epochs=0, pretrain_batch_size=1024, pretrain_lr=None, pretrain_regs=None,
                       pretrain_save=None, pretrain_load=None)
    a = t.parse_args(["--pretrain_epochs", "3", "--pretrain_batch_size", "512", "--pretrain_lr", "0.01", "--pretrain_regs",
                      "1e-5", "--pretrain_save", "a.npz", "--pretrain_load", "b.npz", "--epochs", "0"])
    assert (a.pretrain_epochs, a.pretrain_batch_size, a.pretrain_lr, a.pretrain_regs, a.pretrain_save, a.pretrain_load,
            a.epochs) == (3, 512, 0.01, 1e-5, "a.npz", "b.npz", 0)
    for argv in (["--pretrain_epochs", "2", "--gpus", "2"], ["--pretrain_load", "x.npz", "--gpus", "2"],
                 ["--pretrain_epochs", "-1"], ["--pretrain_epochs", "1", "--pretrain_batch_size", "0"]):
        with pytest.raises(SystemExit):
            t.parse_args(argv)
    capsys.readouterr()
    assert t.parse_args(["--gpus", "2"]).gpus == 2          # (without pretraining: as before)
