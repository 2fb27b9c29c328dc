"""Attention-path explanations (KGAT paper, section 4.5 / figure 4): why is this item recommended to this user?

The answer is the walk of highest attention product from the item to the user through the collaborative knowledge
graph.  Edges run tail -> head (reference dataset.py:116) and information flows along them, so a walk for query q starts
at ``items[q]`` and ends at ``users[q]``.  The arithmetic is a max-times product over the CSR, one launch of
``kgat_spmm_umule_max_f32`` per hop with the queries as columns:

    B_0[items[q], q] = 1, 0 elsewhere
    B_l[v, q] = max over edges e = (u -> v) of  w[e] * B_{l-1}[u, q],     A_l[v, q] = the edge that attains it
    score[q, l - 1] = B_l[users[q], q]           (0: no walk of exactly l edges)

and the walk of length l is read back from A_l, A_{l-1}, ... starting at the user, through the edges' sources: a few
small gathers, no host loop over nodes.  Equal products resolve to the smallest edge id (the kernel's rule), so the
result is a function of the graph and the weights alone.

These are WALKS: a node may repeat.  For max_len <= 3, an item the user has no direct edge with and a graph without
self-loops, every walk found is a simple path.  Weights are expected non-negative (attention or Laplacian weights).

``top`` = 2..4 ranks several walks per length (the paper's figure shows a few scored paths and highlights the best): the
k-best recurrence on ``kgat_spmm_umule_max4_f32``, every (node, query) holding its four best prefixes in order,

    B_0[items[q], q, 0] = 1, 0 elsewhere
    B_l[v, q, 0..3] = the four largest of  w[e] * B_{l-1}[u, q, s]  over edges e = (u -> v) and slots s
    (A_l, S_l)[v, q, r] = the (edge, slot) that attains entry r

Multiplying by w >= 0 is monotone under fp32 rounding, so the four largest products of length l at v are, as values, the
four largest of w_e times the four largest of length l - 1 at the source of e: a prefix outside its node's four is
dominated by four prefixes through the same edge.  Distinct (edge, slot) back-pointers are distinct walks, and the
chain of slot 0 never leaves slot 0: it is the ``top=1`` walk.  The r-th walk of length l is read back from the user's
slot r through (A, S) and the edges' sources.
"""
import torch

from . import ops
from ._lib import KGATLibraryError

_WIDTHS = (16, 32, 64, 128)  # the column counts of the kernel's fast path; queries are padded to the next one
_QUERIES = (4, 8, 16, 32)    # the query counts of the top-4 kernel (four slots each, the same row widths)


class AttentionPaths:
    """Result of ``attention_paths`` for Q queries and walk lengths 1 .. max_len (index l - 1):

    score      (Q, max_len) float32: the attention product of the best walk of exactly l edges, 0 where none exists
    edges      (Q, max_len, max_len) int64: its edge ids in flow order (item first), -1 padded
    nodes      (Q, max_len, max_len + 1) int64: its nodes, ``items[q]`` first and ``users[q]`` last, -1 padded
    relations  edata['type'] of ``edges`` (-1 padded), or None when the graph has no 'type'
    best_len   (Q,) int64: the length with the largest score (the shortest of equals), 0 when no walk exists
    """
    __slots__ = ("score", "edges", "nodes", "relations", "best_len")

    def __init__(self, score, edges, nodes, relations, best_len):
        self.score, self.edges, self.nodes, self.relations, self.best_len = score, edges, nodes, relations, best_len

    def best(self, q):
        """(nodes, relations or None, score) of query q's best walk as python lists / a float; ([], [], 0.0) if none."""
        n = int(self.best_len[q])
        if n == 0:
            return [], ([] if self.relations is not None else None), 0.0
        rel = None if self.relations is None else self.relations[q, n - 1, :n].tolist()
        return self.nodes[q, n - 1, :n + 1].tolist(), rel, float(self.score[q, n - 1])

    def describe(self, q):
        """The best walk of query q as ``node -rel-> node ...`` (``node -> node`` without relations)."""
        nodes, rel, _ = self.best(q)
        return _walk_text(nodes, rel) if nodes else "(no walk)"


def _walk_text(nodes, rel):
    out = [str(nodes[0])]
    for j in range(1, len(nodes)):
        out.append(("-%d->" % rel[j - 1]) if rel is not None else "->")
        out.append(str(nodes[j]))
    return " ".join(out)


class TopAttentionPaths:
    """Result of ``attention_paths(top=K)``, K in 2..4, for Q queries and walk lengths 1 .. max_len (index l - 1); slot r
    is the walk with the r-th largest product among those of exactly l edges (equal products: the kernel's rule):

    score        (Q, max_len, K) float32, descending in the last axis; 0 where fewer than r + 1 walks exist
    edges        (Q, max_len, K, max_len) int64: edge ids in flow order (item first), -1 padded
    nodes        (Q, max_len, K, max_len + 1) int64: ``items[q]`` first and ``users[q]`` last, -1 padded
    relations    edata['type'] of ``edges`` (-1 padded), or None when the graph has no 'type'
    ranked_score (Q, K) float32: the K best walks over all lengths, ordered by (score descending, length ascending,
                 slot ascending); 0 where no further walk exists
    ranked_len   (Q, K) int64: their lengths, 0 for none
    ranked_slot  (Q, K) int64: their slots, -1 for none
    """
    __slots__ = ("score", "edges", "nodes", "relations", "ranked_score", "ranked_len", "ranked_slot")

    def __init__(self, score, edges, nodes, relations, ranked_score, ranked_len, ranked_slot):
        self.score, self.edges, self.nodes, self.relations = score, edges, nodes, relations
        self.ranked_score, self.ranked_len, self.ranked_slot = ranked_score, ranked_len, ranked_slot

    def walk(self, q, r):
        """(nodes, relations or None, score) of query q's walk of rank r as python lists / a float; ([], [], 0.0) if
        there is none."""
        n = int(self.ranked_len[q, r])
        if n == 0:
            return [], ([] if self.relations is not None else None), 0.0
        s = int(self.ranked_slot[q, r])
        rel = None if self.relations is None else self.relations[q, n - 1, s, :n].tolist()
        return self.nodes[q, n - 1, s, :n + 1].tolist(), rel, float(self.ranked_score[q, r])

    def describe(self, q, r):
        """The walk of rank r of query q as ``node -rel-> node ...`` (``node -> node`` without relations)."""
        nodes, rel, _ = self.walk(q, r)
        return _walk_text(nodes, rel) if nodes else "(no walk)"

    def first(self):
        """Slot 0 of every length as an ``AttentionPaths``: what ``top=1`` returns."""
        score = self.score[:, :, 0].contiguous()
        relations = None if self.relations is None else self.relations[:, :, 0].contiguous()
        return AttentionPaths(score, self.edges[:, :, 0].contiguous(), self.nodes[:, :, 0].contiguous(), relations,
                              _best_len(score))


def _best_len(score):
    """(Q,) the length with the largest score of (Q, L), the shortest of equals, 0 when every score is 0."""
    n_q, L = score.shape
    top = score.max(dim=1, keepdim=True).values if n_q else score.new_zeros((0, 1))
    lens = torch.arange(1, L + 1, device=score.device).expand(n_q, L)
    best_len = torch.where(score == top, lens, lens.new_tensor(L + 1)).min(dim=1).values
    return torch.where(top.reshape(-1) > 0, best_len, best_len.new_tensor(0))


def _relations(g, edges, n_edges, dev):
    if "type" not in g.edata:
        return None
    et = g.edata["type"].to(dev).long().reshape(-1)
    return torch.where(edges >= 0, et[edges.clamp(min=0)], edges.new_tensor(-1)) if n_edges else edges.clone()


def _ids(x, n_nodes, name, device):
    t = torch.as_tensor(x, dtype=torch.int64).reshape(-1)
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= n_nodes):
        raise ValueError("%s out of range: node ids must be in [0, %d)" % (name, n_nodes))
    return t.to(device)


def attention_paths(g, w, users, items, max_len=3, top=1):
    """Best attention walks from ``items[q]`` to ``users[q]`` for every query q (equal-length lists of node ids).

    ``w``: the (E,) or (E,1) edge weight in edge-id order on the HIP device - what ``compute_attention`` and
    ``laplacian_weights`` return (a pending lazy weight tensor is read from its CSR copy).  Returns an
    ``AttentionPaths``.  One kernel launch per hop and per chunk of at most 128 queries.  No gradient flows: a weight
    that requires one under grad mode is refused.

    ``top`` in 2..4: the ``top`` best walks of every length and a ranking over all lengths, as a ``TopAttentionPaths``
    (one ``kgat_spmm_umule_max4_f32`` launch per hop and per chunk of at most 32 queries; four slots are always
    computed and ``top`` slices them).  ``top=1`` is the one-winner kernel and result."""
    from .graph import DGLError
    if g.partition is not None:
        raise DGLError("attention_paths on a partitioned graph: a walk crosses shards; use the unsharded graph")
    max_len = int(max_len)
    if max_len < 1:
        raise ValueError("max_len must be >= 1, got %d" % max_len)
    top = int(top)
    if not 1 <= top <= 4:
        raise ValueError("top must be 1, 2, 3 or 4, got %d" % top)
    if not isinstance(w, torch.Tensor) or not w.is_cuda:
        raise KGATLibraryError("attention_paths runs on a HIP device only: the edge weight is %s"
                               % (w.device if isinstance(w, torch.Tensor) else type(w).__name__))
    if torch.is_grad_enabled() and w.requires_grad:
        raise NotImplementedError("attention_paths has no backward: call it under torch.no_grad() or on detached weights")
    st = g._st
    n, dev = st.n_nodes, w.device
    if w.shape[0] != st.n_edges:
        raise ValueError("edge weight has %d rows, graph has %d edges" % (w.shape[0], st.n_edges))
    users, items = _ids(users, n, "users", dev), _ids(items, n, "items", dev)
    if users.numel() != items.numel():
        raise ValueError("users and items must have the same length (%d vs %d)" % (users.numel(), items.numel()))
    n_q, L = users.numel(), max_len
    if top > 1:
        return _attention_paths_top(g, st, w, users, items, L, top)
    with torch.no_grad():
        csr = st.csr(dev)
        w_csr = st.csr_weights(w)
        src = st.coo(dev)[0].long()
        score = torch.zeros((n_q, L), dtype=torch.float32, device=dev)
        edges = torch.full((n_q, L, L), -1, dtype=torch.int64, device=dev)
        nodes = torch.full((n_q, L, L + 1), -1, dtype=torch.int64, device=dev)
        for q0 in range(0, n_q, _WIDTHS[-1]):
            u, it = users[q0:q0 + _WIDTHS[-1]], items[q0:q0 + _WIDTHS[-1]]
            qc = u.numel()
            width = next(d for d in _WIDTHS if d >= qc)
            cols = torch.arange(qc, device=dev)
            b = torch.zeros((n, width), dtype=torch.float32, device=dev)
            b[it, cols] = 1.0
            args = []
            ws = ops.spmm_max_workspace(csr.col.numel(), width, dev)
            for hop in range(L):
                b, a = ops.spmm_max(csr.indptr, csr.col, csr.row_of, b, w_csr, eid=csr.eid, workspace=ws)
                args.append(a)
                score[q0:q0 + qc, hop] = b[u, cols]
            for hop in range(L if st.n_edges else 0):  # the walk of hop + 1 edges, from the user back to the item
                found = score[q0:q0 + qc, hop] != 0
                at = u
                nodes[q0:q0 + qc, hop, hop + 1] = torch.where(found, at, at.new_tensor(-1))
                for j in range(hop, -1, -1):
                    e = args[j][at, cols].long().clamp_(min=0)  # (a query without a walk: any edge, masked below)
                    at = src[e]
                    edges[q0:q0 + qc, hop, j] = torch.where(found, e, e.new_tensor(-1))
                    nodes[q0:q0 + qc, hop, j] = torch.where(found, at, at.new_tensor(-1))
        relations = _relations(g, edges, st.n_edges, dev)
        best_len = _best_len(score)
    return AttentionPaths(score, edges, nodes, relations, best_len)


def _attention_paths_top(g, st, w, users, items, L, top):
    """attention_paths for top in 2..4 (operands checked by the caller)."""
    n, dev, n_q = st.n_nodes, w.device, users.numel()
    with torch.no_grad():
        csr = st.csr(dev)
        w_csr = st.csr_weights(w)
        src = st.coo(dev)[0].long()
        score = torch.zeros((n_q, L, top), dtype=torch.float32, device=dev)
        edges = torch.full((n_q, L, top, L), -1, dtype=torch.int64, device=dev)
        nodes = torch.full((n_q, L, top, L + 1), -1, dtype=torch.int64, device=dev)
        none = torch.tensor(-1, dtype=torch.int64, device=dev)
        for q0 in range(0, n_q, _QUERIES[-1]):
            u, it = users[q0:q0 + _QUERIES[-1]], items[q0:q0 + _QUERIES[-1]]
            qc = u.numel()
            width = next(d for d in _QUERIES if d >= qc)
            cols = torch.arange(qc, device=dev)
            b = torch.zeros((n, width, 4), dtype=torch.float32, device=dev)
            b[it, cols, 0] = 1.0
            back = []
            ws = ops.spmm_max4_workspace(csr.col.numel(), 4 * width, dev)
            for hop in range(L):
                b, a, s = ops.spmm_max4(csr.indptr, csr.col, csr.row_of, b, w_csr, eid=csr.eid, workspace=ws)
                back.append((a, s))
                score[q0:q0 + qc, hop] = b[u, cols, :top]
            cols = cols[:, None]
            for hop in range(L if st.n_edges else 0):  # the walks of hop + 1 edges, from the user back to the item
                found = score[q0:q0 + qc, hop] != 0    # (qc, top)
                at = u[:, None].expand(qc, top)
                slot = torch.arange(top, device=dev).expand(qc, top)
                nodes[q0:q0 + qc, hop, :, hop + 1] = torch.where(found, at, none)
                for j in range(hop, -1, -1):
                    a, s = back[j]
                    e = a[at, cols, slot].long().clamp_(min=0)  # (no such walk: any edge and slot, masked below)
                    slot = s[at, cols, slot].long().clamp_(max=3)
                    at = src[e]
                    edges[q0:q0 + qc, hop, :, j] = torch.where(found, e, none)
                    nodes[q0:q0 + qc, hop, :, j] = torch.where(found, at, none)
        relations = _relations(g, edges, st.n_edges, dev)
        # the ranking over all lengths: a stable descending sort of the (length, slot)-major scores
        ranked_score, idx = torch.sort(score.reshape(n_q, L * top), dim=1, descending=True, stable=True)
        ranked_score, idx = ranked_score[:, :top].contiguous(), idx[:, :top]
        some = ranked_score > 0
        ranked_len = torch.where(some, idx // top + 1, idx.new_tensor(0))
        ranked_slot = torch.where(some, idx % top, idx.new_tensor(-1))
    return TopAttentionPaths(score, edges, nodes, relations, ranked_score, ranked_len, ranked_slot)
