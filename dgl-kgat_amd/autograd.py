"""Autograd glue for the differentiable sparse operators of the path.

* ``u_mul_e_sum`` - update_all(u_mul_e, sum), reference models.py:63.  Backward w.r.t. the
  node features is the same SpMM kernel on the reversed graph's CSR;
  backward w.r.t. the edge weight is an SDDMM (only when the weight requires grad - in the
  reference it never does, kgat.py:142-144).
* ``edge_softmax`` - reference models.py:153; backward as DGL 0.4.x EdgeSoftmax.backward.
* ``copy_reduce`` - update_all(copy_src, sum | mean), the aggregation of DGL's SAGEConv (gnn_model
  "graphsage"); backward over the reversed graph's CSR.
* ``max_reduce`` - update_all(u_mul_e | copy_src, max) (kgat_spmm_umule_max_f32).  Forward only: it lives here to refuse,
  in one place, inputs that would need a backward.
* ``gat_aggregate`` - the message passing of DGL's GATConv (kgat_gat_fwd_f32 / kgat_gat_bwd_f32): logits, destination softmax,
  attention dropout and the weighted sum per head in one walk; backward towards ft, el and er.
* ``rgcn_aggregate`` - the message passing of DGL's RelGraphConv with basis decomposition, aggregate-first
  (kgat_rgcn_fwd_f32 / kgat_rgcn_bwd_x_f32 / kgat_rgcn_bwd_coef_f32): one gather of a source row feeds B accumulators;
  backward towards x and the coefficients.
* ``kgat_attention`` - the fused attention (logits + destination softmax, models.py:135-154) as one unit that
  differentiates towards the entity table, W_R and the relation embeddings.
* ``bi_pool`` - NFM's Bi-Interaction pooling over sparse feature sets (kgat_bi_pool_fwd_f32 / kgat_bi_pool_bwd_f32): the
  operator of the FM and NFM baselines; backward towards the embedding table and the linear weights, dense.
* ``ripple_hop`` - RippleNet's attention of one item vector over a user's ripple set of one hop (kgat_ripple_hop_fwd_f32 /
  kgat_ripple_hop_bwd_f32): logits, softmax and the weighted sum of the tail rows in one walk; backward towards the
  query table and, through two incidence lists summed by the sum kernel, towards the entity table, dense.
"""
import torch
from torch.autograd.function import once_differentiable

from . import ops


class _UMulESum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, g, mul_self):
        st = g._st
        dev = x.device
        x2 = x if x.dim() == 2 else x.unsqueeze(1)
        x2 = x2.contiguous()
        if x2.dtype != torch.float32:
            raise TypeError("node features must be float32, got %s" % x2.dtype)
        csr = st.csr(dev)
        w_csr = st.csr_weights(w)  # a pending lazy attention tensor is served from its CSR copy
        # (a destination-range shard is an ordinary graph holding only its local edges: rows it
        # does not own come out as zeros and the caller exchanges them, partition.py)
        out = ops.spmm(csr.indptr, csr.col, csr.row_of, x2.detach(), w_csr, mul_self=mul_self)
        ctx.g, ctx.mul_self, ctx.squeeze = g, mul_self, x.dim() == 1
        ctx.w_shape = w.shape
        ctx.save_for_backward(x2, w, out if mul_self else None)
        return out.squeeze(1) if x.dim() == 1 else out

    @staticmethod
    def backward(ctx, grad_out):
        x2, w, _ = ctx.saved_tensors
        st = ctx.g._st
        dev = grad_out.device
        if ctx.mul_self:
            raise NotImplementedError("backward of the fused h*h_N epilogue: use the unfused op")
        go = (grad_out.unsqueeze(1) if ctx.squeeze else grad_out).contiguous()
        grad_x = grad_w = None
        if ctx.needs_input_grad[0]:
            rev = st.csr_rev(dev)
            grad_x = ops.spmm(rev.indptr, rev.col, rev.row_of, go, st.rev_weights(w))
            if ctx.squeeze:
                grad_x = grad_x.squeeze(1)
        if ctx.needs_input_grad[1]:
            src, dst = st.coo(dev)
            grad_w = ops.sddmm_dot(src, dst, x2.detach(), go).reshape(ctx.w_shape)
        return grad_x, grad_w, None, None


def u_mul_e_sum(g, x, w, mul_self=False):
    """h_N[v] = sum_{e:u->v} w[e] * x[u]  (optionally * x[v], the bi-interaction product)."""
    if x.shape[0] != g.number_of_nodes():
        raise ValueError("node feature has %d rows, graph has %d nodes" % (x.shape[0], g.number_of_nodes()))
    if w.shape[0] != g.number_of_edges():
        raise ValueError("edge weight has %d rows, graph has %d edges" % (w.shape[0], g.number_of_edges()))
    return _UMulESum.apply(x, w, g, mul_self)


class _CopyReduce(torch.autograd.Function):
    """update_all(copy_src, sum | mean) (kgat_copy_reduce_f32).  Backward w.r.t. the node feature: the sum over the
    reversed graph's CSR - of the incoming gradient itself (sum), or through the aggregation with the weights
    1 / max(in_deg(dst), 1) (mean; kgat_spmm_umule_sum_f32 with a graph-static weight array)."""

    @staticmethod
    def forward(ctx, x, g, reduce):
        st = g._st
        x2 = x if x.dim() == 2 else x.unsqueeze(1)
        x2 = x2.contiguous()
        if x2.dtype != torch.float32:
            raise TypeError("node features must be float32, got %s" % x2.dtype)
        csr = st.csr(x2.device)
        out = ops.copy_reduce(csr.indptr, csr.col, csr.row_of, x2.detach(), reduce)
        ctx.g, ctx.reduce, ctx.squeeze = g, reduce, x.dim() == 1
        return out.squeeze(1) if x.dim() == 1 else out

    @staticmethod
    def backward(ctx, grad_out):
        st = ctx.g._st
        dev = grad_out.device
        go = (grad_out.unsqueeze(1) if ctx.squeeze else grad_out).contiguous()
        rev = st.csr_rev(dev)
        if ctx.reduce == "sum":
            grad_x = ops.copy_reduce(rev.indptr, rev.col, rev.row_of, go, "sum")
        else:
            grad_x = ops.spmm(rev.indptr, rev.col, rev.row_of, go, rev_inv_degree(st, dev))
        return (grad_x.squeeze(1) if ctx.squeeze else grad_x), None, None


def rev_inv_degree(st, device):
    """1 / max(in_deg(v), 1) of every reversed-CSR position's column v (the destination of the forward edge): the
    weights that turn the mean's backward into a weighted sum over the reversed CSR.  Graph-static, cached."""
    c = st._cache(device)
    if "rev_inv_deg" not in c:
        indptr = st.csr(device).indptr
        inv = 1.0 / (indptr[1:] - indptr[:-1]).clamp(min=1).to(torch.float32)
        c["rev_inv_deg"] = inv[st.csr_rev(device).col.long()].contiguous()
    return c["rev_inv_deg"]


def copy_reduce(g, x, reduce="sum"):
    """h_N[v] = sum | mean_{e:u->v} x[u]  (update_all(fn.copy_src, fn.sum | fn.mean))."""
    if x.shape[0] != g.number_of_nodes():
        raise ValueError("node feature has %d rows, graph has %d nodes" % (x.shape[0], g.number_of_nodes()))
    return _CopyReduce.apply(x, g, reduce)


def max_reduce(g, x, w=None):
    """h[v] = max_{e:u->v} w[e] * x[u] (w=None: x[u]) - update_all(fn.u_mul_e | fn.copy_src, fn.max).  There is no
    backward: inputs that would need one are refused, not detached."""
    if x.shape[0] != g.number_of_nodes():
        raise ValueError("node feature has %d rows, graph has %d nodes" % (x.shape[0], g.number_of_nodes()))
    if w is not None and w.shape[0] != g.number_of_edges():
        raise ValueError("edge weight has %d rows, graph has %d edges" % (w.shape[0], g.number_of_edges()))
    if torch.is_grad_enabled() and (x.requires_grad or (w is not None and w.requires_grad)):
        raise NotImplementedError("fn.max has no backward on the HIP kernels: call it under torch.no_grad() or on "
                                  "detached inputs (the feature or the edge weight requires grad)")
    st = g._st
    x2 = (x if x.dim() == 2 else x.unsqueeze(1)).detach().contiguous()
    if x2.dtype != torch.float32:
        raise TypeError("node features must be float32, got %s" % x2.dtype)
    csr = st.csr(x2.device)
    w_csr = None if w is None else st.csr_weights(w)  # a pending lazy attention tensor is served from its CSR copy
    out, _ = ops.spmm_max(csr.indptr, csr.col, csr.row_of, x2, w_csr, want_arg=False)
    return out.squeeze(1) if x.dim() == 1 else out


class _EdgeSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, g):
        st = g._st
        flat = logits.reshape(-1) if (logits.dim() == 1 or (logits.dim() == 2 and logits.shape[1] == 1)) else None
        if flat is None:
            raise NotImplementedError("edge_softmax on the KGAT path takes (E,1) or (E,) logits; got %s"
                                      % (tuple(logits.shape),))
        flat = flat.detach().contiguous()
        if flat.dtype != torch.float32:
            raise TypeError("logits must be float32, got %s" % flat.dtype)
        csr = st.csr(flat.device)
        _, a_csr = ops.edge_softmax(csr.indptr, csr.row_of, csr.eid, flat, want_out=False, want_csr=True)
        a = ops.gather(st.csr_pos(flat.device), a_csr)  # back to edge-id order
        st.remember_weight(a, a_csr)
        ctx.g = g
        ctx.save_for_backward(a)
        return a.reshape(logits.shape)

    @staticmethod
    def backward(ctx, grad_a):
        (a,) = ctx.saved_tensors
        csr = ctx.g._st.csr(a.device)
        gs = ops.edge_softmax_bwd(csr.indptr, csr.eid, a, grad_a.reshape(-1).contiguous())
        return gs.reshape(grad_a.shape), None


def edge_softmax(graph, logits, eids=None):
    """dgl.nn.pytorch.softmax.edge_softmax: normalise `logits` over the incoming edges of each
    destination node.  Output has the shape of the input."""
    if eids is not None:
        raise NotImplementedError("edge_softmax on an edge subset is outside the KGAT path")
    if logits.shape[0] != graph.number_of_edges():
        raise ValueError("logits has %d rows, graph has %d edges" % (logits.shape[0], graph.number_of_edges()))
    return _EdgeSoftmax.apply(logits, graph)


class _KGATAttention(torch.autograd.Function):
    """DGLGraph.kgat_attention under autograd: forward is the default (detached) pipeline - logits of the chosen form,
    kgat_edge_softmax_f32, weights in edge-id order - so the values are its bits; the weights are saved.  Backward:
    kgat_edge_softmax_bwd_f32, one gather of the logit gradients into grouped order, kgat_att_score_bwd_f32 (widths
    outside its range: a torch restatement over the relation-grouped edges)."""

    @staticmethod
    def forward(ctx, ent, W_R, rel, g, etype, algo):
        a = g.kgat_attention(ent, W_R, rel, etype, algo=algo, lazy=False)
        ctx.g, ctx.etype = g, etype
        ctx.save_for_backward(a, ent, W_R, rel)
        return a

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_a):
        from .graph import att_bwd_statics
        a, ent, W_R, rel = ctx.saved_tensors
        st = ctx.g._st
        dev = a.device
        need = ctx.needs_input_grad
        ent_c, W_c, rel_c = ent.detach().contiguous(), W_R.detach().contiguous(), rel.detach().contiguous()
        n_rel, d, k = W_c.shape
        csr = st.csr(dev)
        groups = st.rel_groups(ctx.etype, n_rel, dev)
        gs = ops.edge_softmax_bwd(csr.indptr, csr.eid, a.detach().reshape(-1),
                                  grad_a.detach().reshape(-1).contiguous())
        if ops.att_score_bwd_supported(st.n_nodes, d, k, n_rel):
            s = att_bwd_statics(groups, st.n_nodes)
            g_ent, g_w, g_rel = ops.att_score_bwd(st.n_nodes, s.n_scored, groups.n_groups, groups.perm, groups.src_g, groups.gid,
                                                  s.gstart, groups.gptr, groups.g_node, s.node_ptr, s.node_col,
                                                  s.node_row, s.node_wsrc, ent_c, W_c, rel_c, gs)  # (gathers gs into grouped order)
        else:
            g_ent, g_w, g_rel = _att_score_bwd_torch(groups, ent_c, W_c, rel_c, ops.gather(groups.perm, gs))
        return (g_ent if need[0] else None, g_w if need[1] else None, g_rel if need[2] else None, None, None, None)


def _att_score_bwd_torch(groups, ent, W_R, rel, gamma_g):
    """The logits' backward restated in torch over the relation-grouped edges (one round per relation), for widths
    outside kgat_att_score_bwd_supported: the same gradients to rounding."""
    bounds = groups.rel_ptr.tolist()
    with torch.enable_grad():
        e, w, r = (t.detach().clone().requires_grad_(True) for t in (ent, W_R, rel))
        total = e.sum() * 0 + w.sum() * 0 + r.sum() * 0
        for i in range(w.shape[0]):
            p0, p1 = bounds[i], bounds[i + 1]
            if p1 > p0:
                t_r = e[groups.src_g[p0:p1].long()] @ w[i]
                h_r = e[groups.dst_g[p0:p1].long()] @ w[i]
                total = total + ((t_r * torch.tanh(h_r + r[i])).sum(-1) * gamma_g[p0:p1]).sum()
        return torch.autograd.grad(total, (e, w, r))


def kgat_attention(g, ent, W_R, rel, etype=None, algo="auto"):
    """Differentiable fused attention: the (E,1) weights of ``g.kgat_attention`` in edge-id order, bit for bit, as a
    plain tensor whose grad_fn (when gradients are enabled and `ent`, `W_R` or `rel` requires one) reaches the three
    parameters - what the reference's compute_attention gives without its ``with th.no_grad()`` (models.py:135-154)."""
    if g.partition is not None:
        from .graph import DGLError
        raise DGLError("kgat_attention under autograd on a partitioned graph: a shard holds only part of a tail's "
                       "out-edges; use the unsharded graph")
    if etype is None:
        etype = g.edata["type"]
    return _KGATAttention.apply(ent, W_R, rel, g, etype, algo)


class _TransRLoss(torch.autograd.Function):
    """TransR loss of a triplet batch (reference models.py:114-133).  Forward: the loss, the per-sample rows and the
    weight-gradient partials (kgat_transr_forward_f32); backward: the ordered reductions into the three gradients,
    which read the incoming gradient from device memory (kgat_transr_backward_f32) - no multiply passes."""

    @staticmethod
    def forward(ctx, ent, W_R, rel, h, r, pos_t, neg_t, reg_lambda):
        want = any(ctx.needs_input_grad[:3])
        if not want:
            return ops.transr_loss_grad(h, r, pos_t, neg_t, ent.detach(), W_R.detach(), rel.detach(), reg_lambda,
                                        want_grad=False)[0]
        loss, ws = ops.transr_forward(h, r, pos_t, neg_t, ent.detach(), W_R.detach(), rel.detach(), reg_lambda)
        ctx.ws, ctx.shapes = ws, (tuple(ent.shape), tuple(W_R.shape))
        ctx.save_for_backward(h, r, pos_t, neg_t)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        h, r, pos_t, neg_t = ctx.saved_tensors
        g_ent, g_w, g_rel = ops.transr_backward(h, r, pos_t, neg_t, ctx.shapes, ctx.ws,
                                                grad_scale=grad_out.detach().to(torch.float32))
        need = ctx.needs_input_grad
        return (g_ent if need[0] else None, g_w if need[1] else None, g_rel if need[2] else None,
                None, None, None, None, None)


def transr_loss(ent, W_R, rel, h, r, pos_t, neg_t, reg_lambda):
    """Differentiable fused TransR loss; index tensors of any integer dtype."""
    i32 = [t if t.dtype == torch.int32 and t.is_contiguous() else t.to(torch.int32).contiguous() for t in (h, r, pos_t, neg_t)]
    return _TransRLoss.apply(ent, W_R, rel, *i32, float(reg_lambda))


class _BPRLoss(torch.autograd.Function):
    """BPR loss of the CF phase (reference models.py:170-178) as two launches forward and one sort + one scatter
    backward (kgat_bpr_loss_f32 / kgat_bpr_grad_f32) instead of ~75 torch operator launches; the incoming gradient
    is read by the scatter kernel from device memory."""

    @staticmethod
    def forward(ctx, emb, u, p, n, reg_lambda):
        e = emb.detach()
        loss, coef, ws = ops.bpr_loss(e, u, p, n, reg_lambda)
        ctx.reg_lambda, ctx.ws = reg_lambda, ws
        ctx.save_for_backward(e, u, p, n, coef)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        e, u, p, n, coef = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        g = ops.bpr_grad(e, u, p, n, coef, ctx.reg_lambda, grad_scale=grad_out.detach().to(torch.float32), workspace=ctx.ws)
        return g, None, None, None, None


def bpr_loss(embedding, src_ids, pos_dst_ids, neg_dst_ids, reg_lambda):
    """Differentiable fused BPR loss; index tensors of any integer dtype (int32 is passed through as is)."""
    i32 = [t if t.dtype == torch.int32 and t.is_contiguous() else t.to(torch.int32).contiguous()
           for t in (src_ids, pos_dst_ids, neg_dst_ids)]
    return _BPRLoss.apply(embedding, *i32, float(reg_lambda))


class _GNNTrain(torch.autograd.Function):
    """The whole propagation stack under autograd (reference models.py:156-168 with the KGATConv of
    :49-70 in training mode) as one differentiable unit: per layer the SpMM, one kernel for
    (h * h_N) W2^T + LeakyReLU + dropout + the normalised copy written into its slice of the
    readout; backward per layer one kernel for the normalise / dropout / LeakyReLU gradients, two
    dense GEMMs, one two-product pass and the SpMM on the reversed CSR.  Gradients: the input
    embeddings and every W2; the edge weights are constants (kgat.py:139-145).
    `forms`: each layer's aggregator (ops.FORMS: the product of Bi, the sum of GCN, the concatenation of GraphSage -
    KGATConv's res_type); the backward is routed by it, its structure is the same for all three.  ops.BI2_FORM: the
    paper's two-term Bi-Interaction - such a layer has TWO weights in `weights` (W1 on h + h_N, then W2 on h * h_N), its
    forward also saves the sign record, its backward head writes two gradients, and its backward towards the inputs
    still ends in ONE reversed aggregation.
    `edge` = (edge_p, edge_seed): node dropout - with edge_p > 0 every layer aggregates over ONE dropped adjacency, the
    forward stream ops.edge_dropout(w_csr, csr.eid, ...) formed here, the reversed stream ops.edge_dropout(w_rev,
    csr_rev.eid, ...) formed in backward: keyed by edge id, both hold the same surviving edges.  The edge-id-ordered
    dropped weights are never formed, and the graph's cached copies of the undropped weights are read, not replaced."""

    @staticmethod
    def forward(ctx, g, slope, drop_p, seed, forms, edge, h0, *weights):
        st = g._st
        dev = h0.device
        h = h0.detach().contiguous()
        csr = st.csr(dev)
        ew = g.edata["w"]
        w_csr = st.csr_weights(ew)
        if edge[0] > 0:
            w_csr = ops.edge_dropout(w_csr, csr.eid, edge[0], edge[1])
        first = [0]  # layer li's weights: weights[first[li]:first[li + 1]]
        for f in forms:
            first.append(first[-1] + ops.form_weights(f))
        widths = [h.shape[1]] + [weights[first[li]].shape[0] for li in range(len(forms))]
        out = torch.empty((h.shape[0], sum(widths)), dtype=torch.float32, device=dev)
        # the ego block (out[:, :d] = h0, models.py:159,168) is written by layer 0's dense kernel from the rows it loads
        # anyway (self_out) where the slice allows 16-byte stores; otherwise by a copy here
        ego_in_kernel = len(forms) > 0 and widths[0] % 4 == 0 and out.shape[1] % 4 == 0 and h.shape[0] > 0
        if not ego_in_kernel:
            out[:, :widths[0]] = h
        off = widths[0]
        hs, hns, signs = [h], [], []
        for li, form in enumerate(forms):
            hn = ops.spmm(csr.indptr, csr.col, csr.row_of, hs[-1], w_csr)
            # (a two-term layer also returns its sign record)
            y, *sg = _each(ops.aggregator_train(form, hs[-1], hn, _layer_weights(weights, first, li), slope, drop_p,
                                                seed + li, norm_out=out[:, off:off + widths[li + 1]],
                                                self_out=out[:, :widths[0]] if (li == 0 and ego_in_kernel) else None))
            signs += sg
            hs.append(y)
            hns.append(hn)
            off += widths[li + 1]
        ctx.g, ctx.slope, ctx.drop_p, ctx.seed, ctx.widths, ctx.ew, ctx.forms = g, slope, drop_p, seed, widths, ew, forms
        ctx.first, ctx.edge = first, edge
        ctx.save_for_backward(*hs, *hns, *weights, *signs)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        n_l = len(ctx.widths) - 1
        saved = ctx.saved_tensors
        first = ctx.first
        hs, hns, weights = saved[:n_l + 1], saved[n_l + 1:2 * n_l + 1], saved[2 * n_l + 1:2 * n_l + 1 + first[-1]]
        signs = list(saved[2 * n_l + 1 + first[-1]:])  # the two-term layers' sign records, in layer order
        st = ctx.g._st
        dev = grad_out.device
        rev = st.csr_rev(dev)
        w_rev = st.rev_weights(ctx.ew)
        if ctx.edge[0] > 0:
            w_rev = ops.edge_dropout(w_rev, rev.eid, ctx.edge[0], ctx.edge[1])
        grad_out = grad_out.contiguous()
        offs = [0]
        for wd in ctx.widths:
            offs.append(offs[-1] + wd)
        g_a = g_b = None  # the two addends of the gradient arriving at hs[li + 1] from the layer above
        grad_w = [None] * first[-1]
        pending = []  # (index into weights, that weight gradient's per-workgroup partials)
        for li in range(n_l - 1, -1, -1):
            form, wi, h, hn = ctx.forms[li], first[li], hs[li], hns[li]
            n_w = first[li + 1] - wi
            # one gradient per weight: grad_z, or (gz1, gz2) from the two-term layer's sign record
            gz = ops.aggregator_bwd_pre(form, hs[li + 1], signs.pop() if n_w == 2 else None, g_a, g_b,
                                        grad_out[:, offs[li + 1]:offs[li + 2]], ctx.slope, ctx.drop_p, ctx.seed + li)
            kernels = ops.aggregator_bwd_supported(form, h.shape[1], _each(gz)[0].shape[1])
            if any(ctx.needs_input_grad[7 + wi:7 + wi + n_w]):
                if kernels:
                    # grad_z^T (h * h_N) (h + h_N, [h | h_N]; both of the two-term layer) as per-workgroup partials;
                    # every layer's set is summed by ONE launch at the end
                    parts = ops.aggregator_bwd_weight(form, gz, h, hn, want_partials=True)
                    pending += [(wi + k, p) for k, p in enumerate(_each(parts))]
                else:
                    for k, (g, x) in enumerate(zip(_each(gz), _combine(form, h, hn))):
                        grad_w[wi + k] = tall_weight_grad(g, x)
            w_l = _layer_weights(weights, first, li)
            if kernels:
                # grad_P = grad_z W formed per tile: the part to be aggregated (grad_P * h for Bi) and the part that goes to
                # h directly (grad_P * h_N); the two-term layer: P1 + P2 * h and P1 + P2 * h_N, P1 = gz1 W1, P2 = gz2 W2
                t, g_b = ops.aggregator_bwd_input(form, gz, w_l, h, hn)
            elif form == ops.BI2_FORM:
                p1, p2 = gz[0] @ w_l[0], gz[1] @ w_l[1]
                t, g_b = p1 + p2 * h, p1 + p2 * hn
            elif form == ops.FORMS["Bi"]:
                t, g_b = ops.mul2(gz @ w_l, h, hn)
            elif form == ops.FORMS["GCN"]:
                t = g_b = gz @ w_l
            else:
                gp, d_in = gz @ w_l, h.shape[1]
                t, g_b = gp[:, d_in:].contiguous(), gp[:, :d_in].contiguous()
            g_a = ops.spmm(rev.indptr, rev.col, rev.row_of, t, w_rev)
        if pending:
            for (wi, _), summed in zip(pending, ops.sum_partials([p_ for _, p_ in pending])):
                grad_w[wi] = summed
        grad_h0 = None
        if ctx.needs_input_grad[6]:
            g0 = grad_out[:, :ctx.widths[0]]
            if g_a is not None and ctx.widths[0] % 4 == 0 and grad_out.shape[1] % 4 == 0 and g0.data_ptr() % 16 == 0:
                grad_h0 = ops.add3_rows(g0, g_a, g_b)      # one pass: (g0 + g_a) + g_b, the same additions
            else:
                grad_h0 = g0 + g_a
                grad_h0 += g_b
        return (None, None, None, None, None, None, grad_h0, *grad_w)


def _each(x):
    """A per-weight value - one tensor, or the two-term layer's pair - as a tuple."""
    return tuple(x) if isinstance(x, (tuple, list)) else (x,)


def _layer_weights(weights, first, li):
    """Layer li's weight out of the flat list, detached: a tensor, or the two-term layer's pair (ops' convention)."""
    ws = tuple(w.detach().contiguous() for w in weights[first[li]:first[li + 1]])
    return ws if len(ws) == 2 else ws[0]


def _combine(form, h, hn):
    """The A operand of each of the layer's weights: h * h_N (Bi), h + h_N (GCN), [h | h_N] (GraphSage), both the sum
    and the product (two-term)."""
    if form == ops.BI2_FORM:
        return h + hn, h * hn
    if form == ops.FORMS["GCN"]:
        return (h + hn,)
    if form == ops.FORMS["GraphSage"]:
        return (torch.cat([h, hn], 1),)
    return (h * hn,)


def tall_weight_grad(grad, x, slabs=128):
    """grad^T @ x for tall operands (N ~ 10^5 rows, <= 128 columns) reducing over N into a tiny
    result: a batched GEMM over row slabs plus a sum (the library's single GEMM for this shape takes
    0.45-0.5 ms at N = 159k; this takes ~30 us)."""
    n = x.shape[0]
    m = (n // slabs) * slabs
    if m < 16 * slabs:
        return grad.t() @ x
    gw = torch.bmm(grad[:m].view(slabs, m // slabs, -1).transpose(1, 2), x[:m].view(slabs, m // slabs, -1)).sum(0)
    if m < n:
        gw = gw + grad[m:].t() @ x[m:]
    return gw


def gnn_train(g, h0, weights, slope=0.01, drop_p=0.0, seed=0, forms=None, edge_drop_p=0.0, edge_seed=0):
    """Differentiable fused propagation stack; returns the (N, sum of widths) readout.  `forms`: one ops.FORMS value per
    layer (default: Bi everywhere); a GraphSage layer's weight is (d_out, 2 d_in).  A two-term layer (ops.BI2_FORM) gives
    its entry of `weights` as the pair (W1, W2) = (res_fc.weight, res_fc_2.weight).  `edge_drop_p` > 0: node dropout
    - the stack, forward and backward, runs over the adjacency dropped with ops.edge_keep_mask(edge_seed, E, edge_drop_p)."""
    forms = tuple(int(f) for f in forms) if forms is not None else (ops.FORMS["Bi"],) * len(weights)
    if len(forms) != len(weights):
        raise ValueError("gnn_train: %d forms for %d layers" % (len(forms), len(weights)))
    if not 0.0 <= float(edge_drop_p) < 1.0:
        raise ValueError("gnn_train: edge_drop_p must be in [0, 1), got %r" % (edge_drop_p,))
    flat = []
    for f, w in zip(forms, weights):
        if f == ops.BI2_FORM:
            if not (isinstance(w, (tuple, list)) and len(w) == 2):
                raise ValueError("gnn_train: a two-term layer takes the pair (W1, W2)")
            flat += list(w)
        else:
            flat.append(w)
    return _GNNTrain.apply(g, float(slope), float(drop_p), int(seed), forms, (float(edge_drop_p), int(edge_seed)), h0,
                           *flat)


class _GATAggregate(torch.autograd.Function):
    """GATConv's aggregation (kgat_gat_fwd_f32) and its backward (kgat_gat_bwd_f32).  Saved: ft, el, er, out and the
    (N, H) row maximum and denominator; nothing edge-sized."""

    @staticmethod
    def forward(ctx, ft, el, er, g, slope, p, seed):
        st = g._st
        ftc, elc, erc = ft.detach().contiguous(), el.detach().contiguous(), er.detach().contiguous()
        out, m, l = ops.gat_forward(st.csr(ftc.device), ftc, elc, erc, slope, p, seed)
        ctx.g, ctx.slope, ctx.p, ctx.seed = g, slope, p, seed
        ctx.save_for_backward(ftc, elc, erc, m, l, out)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        ft, el, er, m, l, out = ctx.saved_tensors
        st = ctx.g._st
        dev = g_out.device
        g_ft, g_el, g_er = ops.gat_backward(st.csr(dev), st.csr_rev(dev), ft, el, er, m, l, out, g_out.contiguous(),
                                            ctx.slope, ctx.p, ctx.seed)
        need = ctx.needs_input_grad
        return (g_ft if need[0] else None, g_el if need[1] else None, g_er if need[2] else None, None, None, None, None)


def _gat_restated(st, ft, el, er, slope, p, seed):
    """The aggregation restated in torch operators over the COO (under torch's autograd), for (H, F) outside
    ops.gat_supported: the same values to rounding, in the kernel's order - the weighted sum of exp(s - m) first, one
    division by the denominator per output element.  torch's scatter adds are unordered atomics, so the arithmetic runs in
    fp64 (forward and, through the casts, backward) and the results are rounded to fp32 once: their order then shows in
    the last bit at most, where in fp32 it showed as several ulps on a hub's gradient."""
    dev = ft.device
    n, H, _ = ft.shape
    src, dst = (t.long() for t in st.coo(dev))
    ft64, el64, er64 = ft.double(), el.double(), er.double()
    s = torch.nn.functional.leaky_relu(el64[src] + er64[dst], slope)
    m = torch.full((n, H), float("-inf"), dtype=torch.float64, device=dev).scatter_reduce(
        0, dst.unsqueeze(1).expand(-1, H), s.detach(), "amax")
    pe = torch.exp(s - m[dst])
    l = torch.zeros((n, H), dtype=torch.float64, device=dev).index_add(0, dst, pe)
    if p > 0:
        keep = torch.as_tensor(ops.dropout_keep_mask(seed, src.numel(), H, p), device=dev)
        cpe = pe * keep.to(pe.dtype) * (1.0 / (1.0 - p))
    else:
        cpe = pe
    num = torch.zeros_like(ft64).index_add(0, dst, cpe.unsqueeze(-1) * ft64[src])
    return (num / torch.where(l > 0, l, torch.ones_like(l)).unsqueeze(-1)).to(ft.dtype)  # (rows without in-edges: 0 / 1)


def gat_aggregate(g, ft, el, er, negative_slope=0.2, attn_drop=0.0, seed=0):
    """rst[v,h,:] = sum_{e:u->v} attn_drop(a)[e,h] * ft[u,h,:] with a = edge_softmax(leaky_relu(el[u] + er[v])) per
    head: the message passing of DGL's GATConv as one differentiable unit (gradients to ft, el and er).  ft (N, H, F),
    el, er (N, H) float32.  The attention is never formed as an edge tensor; attn_drop keeps edge e, head h iff
    ops.dropout_keep_mask(seed, E, H, attn_drop)[e, h]."""
    if ft.dim() != 3 or tuple(el.shape) != tuple(ft.shape[:2]) or tuple(er.shape) != tuple(ft.shape[:2]):
        raise ValueError("gat_aggregate: ft must be (N, H, F) and el, er (N, H); got %s, %s, %s"
                         % (tuple(ft.shape), tuple(el.shape), tuple(er.shape)))
    if ft.shape[0] != g.number_of_nodes():
        raise ValueError("node feature has %d rows, graph has %d nodes" % (ft.shape[0], g.number_of_nodes()))
    if g.partition is not None:
        from .graph import DGLError
        raise DGLError("gat_aggregate on a partitioned graph is not supported: a shard holds only part of a source's "
                       "out-edges; use the unsharded graph")
    for name, t in (("ft", ft), ("el", el), ("er", er)):
        if not t.is_cuda:
            raise ops.KGATLibraryError("%s is on %s: the graph attention only runs on a HIP device (no CPU "
                                       "implementation exists in this package)" % (name, t.device))
        if t.dtype != torch.float32:
            raise TypeError("%s must be float32, got %s" % (name, t.dtype))
    if not 0.0 <= float(attn_drop) < 1.0:
        raise ValueError("gat_aggregate: attn_drop must be in [0, 1), got %r" % (attn_drop,))
    if not 0.0 <= float(negative_slope) <= 1.0:
        raise ValueError("gat_aggregate: negative_slope must be in [0, 1], got %r" % (negative_slope,))
    if ops.gat_supported(ft.shape[1], ft.shape[2]):
        return _GATAggregate.apply(ft, el, er, g, float(negative_slope), float(attn_drop), int(seed))
    return _gat_restated(g._st, ft, el, er, float(negative_slope), float(attn_drop), int(seed))


class _RGCNAggregate(torch.autograd.Function):
    """The relational aggregation (kgat_rgcn_fwd_f32) and its two backward walks (kgat_rgcn_bwd_x_f32,
    kgat_rgcn_bwd_coef_f32).  Saved: x and the coefficients; nothing edge-sized beyond the graph's cached streams."""

    @staticmethod
    def forward(ctx, x, coef, g, etypes, norm):
        st = g._st
        xc, ac = x.detach().contiguous(), coef.detach().contiguous()
        et_csr, nm_csr, _, _ = st.rel_streams(etypes, norm, xc.device)
        Z = ops.rgcn_forward(st.csr(xc.device), et_csr, nm_csr, xc, ac)
        ctx.g, ctx.etypes, ctx.norm = g, etypes, norm
        ctx.save_for_backward(xc, ac)
        return Z

    @staticmethod
    @once_differentiable
    def backward(ctx, g_Z):
        x, a = ctx.saved_tensors
        st = ctx.g._st
        dev = g_Z.device
        g_Z = g_Z.contiguous()
        et_csr, nm_csr, et_rev, nm_rev = st.rel_streams(ctx.etypes, ctx.norm, dev)
        g_x = g_a = None
        if ctx.needs_input_grad[0]:
            g_x = ops.rgcn_backward_x(st.csr_rev(dev), et_rev, nm_rev, g_Z, a)
        if ctx.needs_input_grad[1]:
            g_a = ops.rgcn_backward_coef(st.csr(dev), et_csr, nm_csr, x, g_Z, a.shape[0], a.shape[1])
        return g_x, g_a, None, None, None


def _rgcn_restated(st, x, coef, etypes, norm):
    """The aggregation restated in torch operators over the COO (under torch's autograd), for shapes outside
    ops.rgcn_supported.  torch's scatter adds are unordered atomics, so the arithmetic runs in fp64 (forward and, through
    the casts, backward) and the results are rounded to fp32 once, as _gat_restated does and for the same reason.  One
    index_add per basis: nothing of size E x B x D is formed."""
    dev = x.device
    src, dst = (t.long() for t in st.coo(dev))
    et = etypes.reshape(-1).to(device=dev, dtype=torch.long)
    x64, a64 = x.double(), coef.double()
    ok = ((et >= 0) & (et < coef.shape[0])).to(torch.float64)
    c = a64[et.clamp(0, coef.shape[0] - 1)] * ok.unsqueeze(1)              # (E, B)
    if norm is not None:
        c = c * norm.detach().reshape(-1, 1).to(device=dev, dtype=torch.float64)
    xs = x64[src]
    Z = torch.stack([torch.zeros_like(x64).index_add(0, dst, c[:, b:b + 1] * xs) for b in range(coef.shape[1])], 1)
    return Z.to(x.dtype)


def rgcn_aggregate(g, x, coef, etypes, norm=None):
    """Z[v, b, :] = sum_{e: u->v} norm[e] * coef[etypes[e], b] * x[u, :]: the message passing of DGL's RelGraphConv
    (basis regularizer) aggregate-first, as one differentiable unit (gradients to x and coef).  x (N, D), coef (R, B)
    float32, etypes (E,) integer and norm (E,) or (E, 1) float32 (or None: 1) in edge-id order.  The layer's output is
    Z.view(N, B * D) @ weight.view(B * D, out)."""
    if x.dim() != 2 or coef.dim() != 2:
        raise ValueError("rgcn_aggregate: x must be (N, D) and coef (R, B); got %s, %s" % (tuple(x.shape), tuple(coef.shape)))
    if x.shape[0] != g.number_of_nodes():
        raise ValueError("node feature has %d rows, graph has %d nodes" % (x.shape[0], g.number_of_nodes()))
    e = g.number_of_edges()
    if etypes.dim() != 1 or etypes.shape[0] != e:
        raise ValueError("rgcn_aggregate: etypes must be (E,) = (%d,), got %s" % (e, tuple(etypes.shape)))
    if norm is not None and tuple(norm.shape) not in ((e,), (e, 1)):
        raise ValueError("rgcn_aggregate: norm must be (E,) or (E, 1) with E = %d, got %s" % (e, tuple(norm.shape)))
    if g.partition is not None:
        from .graph import DGLError
        raise DGLError("rgcn_aggregate on a partitioned graph is not supported: a shard holds only part of a source's "
                       "out-edges; use the unsharded graph")
    if norm is not None and norm.requires_grad:
        raise NotImplementedError("rgcn_aggregate: a gradient towards norm is not formed (the normaliser is a constant "
                                  "of the graph)")
    floats = (("x", x), ("coef", coef)) + ((("norm", norm),) if norm is not None else ())
    for name, t in floats:
        if t.dtype != torch.float32:
            raise TypeError("%s must be float32, got %s" % (name, t.dtype))
    if etypes.is_floating_point() or etypes.dtype == torch.bool:
        raise TypeError("etypes must be an integer tensor, got %s" % (etypes.dtype,))
    for name, t in floats:
        if not t.is_cuda:
            raise ops.KGATLibraryError("%s is on %s: the relational aggregation only runs on a HIP device (no CPU "
                                       "implementation exists in this package)" % (name, t.device))
    if ops.rgcn_supported(x.shape[1], coef.shape[1], coef.shape[0]):
        return _RGCNAggregate.apply(x, coef, g, etypes, norm)
    return _rgcn_restated(g._st, x, coef, etypes, norm)


class _BiPool(torch.autograd.Function):
    """Bi-Interaction pooling of feature sets (kgat_bi_pool_fwd_f32) and its dense backward (kgat_bi_pool_bwd_f32)."""

    @staticmethod
    def forward(ctx, V, w_lin, feats, items, extra):
        S, bi, lin, sq = ops.bi_pool_fwd(V.detach(), None if w_lin is None else w_lin.detach(), feats, items, extra)
        if lin is None:
            lin = torch.zeros(items.numel(), dtype=V.dtype, device=V.device)
        ctx.feats, ctx.has_w = feats, w_lin is not None
        ctx.save_for_backward(V, S, items, extra)
        ctx.set_materialize_grads(False)   # an output the loss does not use arrives as None: the entry's NULL path
        return bi, lin, sq

    @staticmethod
    @once_differentiable
    def backward(ctx, g_bi, g_lin, g_sq):
        V, S, items, extra = ctx.saved_tensors
        need_V, need_w = ctx.needs_input_grad[0], ctx.has_w and ctx.needs_input_grad[1]
        if not need_V:   # (the linear term alone: its gradient does not read V)
            g_bi = g_sq = None
        g = [None if t is None else t.to(torch.float32).contiguous() for t in (g_bi, g_lin if need_w else None, g_sq)]
        grad_V, grad_w = ops.bi_pool_bwd(V.detach(), ctx.feats, items, extra, S, *g, want_w=need_w)
        return grad_V if need_V else None, grad_w if need_w else None, None, None, None


def bi_pool(V, w_lin, feats, items, extra=None):
    """NFM's Bi-Interaction pooling over sparse feature sets, differentiable towards V and w_lin: pooled set m is
    ``[extra[m]] + feats[items[m]]`` (extra first; ``extra[m] = -1`` or ``extra=None``: no extra) and the outputs are
    ``bi[m] = ((sum_f v_f)^2 - sum_f v_f^2) / 2`` (n_sets, d), ``lin[m] = sum_f w_lin[f]`` and ``sq[m] = sum_f |v_f|^2``
    (n_sets each; an empty set gives zeros; ``w_lin=None``: lin is zero).  `feats`: an ``fm_models.FeatureSets``; `items`
    item positions, `extra` feature ids, any integer dtype.  On a HIP device in fp32 at a size ``ops.bi_pool_supported``
    takes, one kernel forward and a sort plus one kernel backward, with fixed orders of addition (bitwise reproducible,
    dense gradients whose untouched rows are 0); CPU tensors, other dtypes and sizes run ``fm_models.bi_pool_torch``."""
    from .fm_models import _kernels_apply, bi_pool_torch
    if V.dim() != 2:
        raise ValueError("bi_pool: V must be (n_features, d), got %s" % (tuple(V.shape),))
    if not _kernels_apply(V, w_lin, items.numel()):
        return bi_pool_torch(V, w_lin, feats, items, extra)

    def i32(t):
        return t if t.dtype == torch.int32 and t.is_contiguous() else t.to(torch.int32).contiguous()
    return _BiPool.apply(V, w_lin, feats.to(V.device), i32(items.to(V.device)), None if extra is None else i32(extra.to(V.device)))


class _RippleHop(torch.autograd.Function):
    """Ripple-set attention of one hop (kgat_ripple_hop_fwd_f32), its backward towards the query table
    (kgat_ripple_hop_bwd_f32) and towards the entity table (ops.ripple_scatter)."""

    @staticmethod
    def forward(ctx, ent, U, sets, users, hop):
        o, p = ops.ripple_hop_fwd(ent.detach(), U.detach(), sets, users, hop)
        ctx.sets, ctx.hop = sets, hop
        ctx.save_for_backward(ent, U, users, p)
        return o

    @staticmethod
    @once_differentiable
    def backward(ctx, g_o):
        ent, U, users, p = ctx.saved_tensors
        need_ent, need_U = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        g_o = g_o.to(torch.float32).contiguous()
        grad_U, gl = ops.ripple_hop_bwd(ent.detach(), U.detach(), ctx.sets, users, ctx.hop, p, g_o)
        grad_ent = ops.ripple_scatter(U.detach(), ctx.sets, users, ctx.hop, p, gl, g_o) if need_ent else None
        return grad_ent, grad_U if need_U else None, None, None, None


def ripple_hop_torch(ent, U, sets, users, hop, want_p=False):
    """``ripple_hop`` in torch operators (index_select / softmax, index_add_ under autograd), differentiable: what the
    kernels are compared with and what runs on the CPU, in float64 and outside ``ops.ripple_supported``.  Returns o, or
    (o, p)."""
    dev = ent.device
    sets = sets.to(dev)
    ul = torch.as_tensor(users, device=dev).long()
    b, M, R = ul.numel(), sets.n_memory, sets.n_rel
    h, r, t = (getattr(sets, name)[ul, int(hop)].long() for name in ("mem_h", "mem_r", "mem_t"))
    H = ent.index_select(0, h.reshape(-1)).view(b, M, -1)
    q = (torch.arange(b, device=dev).unsqueeze(1) * R + r).reshape(-1)
    Q = U.reshape(b * R, -1).index_select(0, q).view(b, M, -1)
    p = torch.softmax((H * Q).sum(-1), 1)
    T = ent.index_select(0, t.reshape(-1)).view(b, M, -1)
    o = (p.unsqueeze(-1) * T).sum(1)
    return (o, p) if want_p else o


def ripple_kernels_apply(ent, U, sets):
    """Whether ``ripple_hop`` takes the kernels: fp32 on a HIP device, contiguous, 16-byte aligned, a supported size."""
    return (ent.is_cuda and ent.dtype == torch.float32 and U.dtype == torch.float32 and ent.is_contiguous() and
            ent.data_ptr() % 16 == 0 and U.shape[0] >= 1 and
            ops.ripple_supported(ent.shape[1], sets.n_memory, sets.n_rel, U.shape[0]))


def ripple_hop(ent, U, sets, users, hop):
    """RippleNet's attention of one hop, differentiable towards ent and U: for sample b with user ``users[b]`` and the
    hop's ripple set (h_i, r_i, t_i), ``s_i = <U[b, r_i], ent[h_i]>``, ``p = softmax(s)``, ``o[b] = sum_i p_i ent[t_i]``
    (n_samples, d).  `sets`: a ``ripple_models.RippleSets``; U (n_samples, n_rel, d) with ``U[b, r] = v_b R_r``; `users`
    any integer dtype.  On a HIP device in fp32 at a size ``ops.ripple_supported`` takes: one kernel forward, one kernel
    plus two csr_from_coo + spmm sums backward, with fixed orders of addition (bitwise reproducible, dense gradients
    whose untouched rows are 0); CPU tensors, other dtypes and sizes run ``ripple_hop_torch``."""
    if ent.dim() != 2 or U.dim() != 3 or U.shape[1] != sets.n_rel or U.shape[2] != ent.shape[1]:
        raise ValueError("ripple_hop: ent must be (n_nodes, d) and U (n_samples, %d, d), got %s and %s"
                         % (sets.n_rel, tuple(ent.shape), tuple(U.shape)))
    if not 0 <= int(hop) < sets.n_hop:
        raise ValueError("ripple_hop: hop %d outside [0, %d)" % (hop, sets.n_hop))
    if not ripple_kernels_apply(ent, U, sets):
        return ripple_hop_torch(ent, U, sets, users, hop)
    users = torch.as_tensor(users, device=ent.device)
    if users.dtype != torch.int32 or not users.is_contiguous():
        users = users.to(torch.int32).contiguous()
    return _RippleHop.apply(ent, U.contiguous(), sets.to(ent.device), users, int(hop))
