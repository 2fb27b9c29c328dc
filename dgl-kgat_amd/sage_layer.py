"""GraphSAGE (mean aggregator) on the HIP kernels: ``SAGEConv`` is what ``dgl.nn.pytorch.conv.SAGEConv`` resolves to
after ``compat.install_as_dgl()``, so the reference's ``Model(..., gnn_model="graphsage")`` (models.py:98-100,107-109)
builds, trains and evaluates over this package.

Semantics of DGL 0.4.x ``SAGEConv(in_feats, out_feats, aggregator_type="mean", feat_drop, bias, norm, activation)``
on a homogeneous graph:

    hd = feat_drop(h);  h_neigh[v] = mean_{u->v} hd[u] (0 without in-edges);  rst = fc_self(hd) + fc_neigh(h_neigh)
    rst = activation(rst) if activation; rst = norm(rst) if norm

with ``fc_self`` / ``fc_neigh`` ``nn.Linear(in_feats, out_feats, bias)``, weights xavier-uniform (gain of relu), so a
state_dict of a DGL run loads unchanged.  The dropout is this package's counter-hash mask (the precedent of
``KGATConv.mess_drop``): layer i of a stack draws it from ``(seed + i, row, column)`` of its input,
``ops.dropout_keep_mask(seed + i, N, d_in, p)`` reproduces it.

Per layer: ``kgat_dropout_rows_f32`` (when p > 0), ``kgat_copy_reduce_f32`` (mean), ``kgat_sage_dense_f32`` (both
products, the biases and a ReLU in one launch); the backward is ``kgat_bi_interaction_bwd_pre_f32`` (ReLU / identity
gradient), ``kgat_sage_bwd_input_f32``, ``kgat_copy_reduce_f32`` (sum over the reversed CSR), ``kgat_dropout_rows_f32``
(the mask again, and the sum of the two gradient paths) and ``kgat_sage_bwd_weight_f32`` + ``kgat_sum_partials_f32``.
Widths outside {16, 32, 64, 128} take ``F.linear`` for the dense part only."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops


def fusable_activation(act):
    """None / 'relu' for an activation the dense kernel applies itself, or False."""
    if act is None:
        return None
    if act is F.relu or act is torch.relu or isinstance(act, nn.ReLU):
        return "relu"
    return False


def draw_seed():
    """One draw from torch's CPU generator (torch.manual_seed reproduces a run), as KGATPropagation.gnn draws the
    bi-interaction's dropout seed."""
    return int(torch.empty((), dtype=torch.int64).random_())


class _SAGELayer(torch.autograd.Function):
    """One SAGEConv (mean) forward over the kernels; saves hd, h_neigh and Z for the backward."""

    @staticmethod
    def forward(ctx, h, W_s, b_s, W_n, b_n, g, p, seed, act):
        st = g._st
        dev = h.device
        csr = st.csr(dev)
        hc = h.detach().contiguous()
        hd = ops.dropout_rows(hc, p, seed) if p > 0 else hc
        hn = ops.copy_reduce(csr.indptr, csr.col, csr.row_of, hd, "mean")
        z = ops.sage_dense(hd, hn, W_s.detach(), W_n.detach(), None if b_s is None else b_s.detach(),
                           None if b_n is None else b_n.detach(), act)
        ctx.g, ctx.p, ctx.seed, ctx.act = g, p, seed, act
        ctx.save_for_backward(hd, hn, z, W_s, W_n)
        return z

    @staticmethod
    def backward(ctx, gz):
        hd, hn, z, W_s, W_n = ctx.saved_tensors
        st = ctx.g._st
        dev = gz.device
        need = ctx.needs_input_grad
        # gradient at the pre-activation: ReLU' from the saved output (slope 0), identity (slope 1)
        gpre = ops.bi_interaction_bwd_pre(z, gz.contiguous(), None, None, 0.0 if ctx.act == "relu" else 1.0, 0.0, 0)
        gh = gWs = gbs = gWn = gbn = None
        if need[0]:
            g_self, g_agg = ops.sage_bwd_input(gpre, W_s.detach(), W_n.detach(), st.csr(dev).indptr)
            rev = st.csr_rev(dev)
            g_rev = ops.copy_reduce(rev.indptr, rev.col, rev.row_of, g_agg, "sum")
            gh = ops.dropout_rows(g_self, ctx.p, ctx.seed, x2=g_rev)  # (p = 0: the sum of the two paths)
        if any(need[1:5]):
            gWs, gWn, gb = ops.sage_bwd_weight(gpre, hd, hn)
            gWs = gWs if need[1] else None
            gWn = gWn if need[3] else None
            gbs = gb if need[2] else None
            gbn = gb.clone() if need[4] else None
        return gh, gWs, gbs, gWn, gbn, None, None, None, None


class _DropoutRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed):
        ctx.p, ctx.seed = p, seed
        return ops.dropout_rows(x.detach().contiguous(), p, seed)

    @staticmethod
    def backward(ctx, g):
        return ops.dropout_rows(g.contiguous(), ctx.p, ctx.seed), None, None


class SAGEConv(nn.Module):
    """dgl.nn.pytorch.conv.SAGEConv with ``aggregator_type="mean"`` (DGL 0.4.x) on the HIP kernels."""

    def __init__(self, in_feats, out_feats, aggregator_type, feat_drop=0.0, bias=True, norm=None, activation=None):
        super().__init__()
        if isinstance(in_feats, (tuple, list)):
            raise NotImplementedError("SAGEConv: bipartite (tuple) inputs are not supported; only homogeneous graphs")
        if aggregator_type != "mean":
            raise NotImplementedError("SAGEConv: aggregator_type %r is not supported; only 'mean' runs on the HIP "
                                      "kernels (the reference's graphsage model uses 'mean')" % (aggregator_type,))
        self._in_feats = self._in_src_feats = self._in_dst_feats = in_feats
        self._out_feats = out_feats
        self._aggre_type = aggregator_type
        self.norm = norm
        self.feat_drop = nn.Dropout(feat_drop)
        self.activation = activation
        self.fc_self = nn.Linear(in_feats, out_feats, bias=bias)
        self.fc_neigh = nn.Linear(in_feats, out_feats, bias=bias)
        self.reset_parameters()

    def reset_parameters(self):
        gain = nn.init.calculate_gain("relu")
        nn.init.xavier_uniform_(self.fc_self.weight, gain=gain)
        nn.init.xavier_uniform_(self.fc_neigh.weight, gain=gain)

    def drop_p(self):
        return self.feat_drop.p if self.training else 0.0

    def fused_activation(self):
        """None / 'relu' when the dense kernel applies the activation, False otherwise."""
        return fusable_activation(self.activation)

    def forward(self, graph, feat, seed=None):
        from .graph import DGLError
        if isinstance(feat, (tuple, list)):
            raise NotImplementedError("SAGEConv: bipartite (tuple) inputs are not supported")
        if graph.partition is not None:
            raise DGLError("SAGEConv on a partitioned graph is not supported (sharded GraphSAGE is out of scope)")
        if feat.shape[0] != graph.number_of_nodes():
            raise ValueError("node feature has %d rows, graph has %d nodes" % (feat.shape[0], graph.number_of_nodes()))
        p = self.drop_p()
        if p > 0 and seed is None:
            seed = draw_seed()
        seed = 0 if seed is None else int(seed)
        act = self.fused_activation()
        d_in, d_out = self._in_feats, self._out_feats
        if ops.sage_dense_supported(d_in, d_out) and feat.is_cuda:
            rst = _SAGELayer.apply(feat, self.fc_self.weight, self.fc_self.bias, self.fc_neigh.weight,
                                   self.fc_neigh.bias, graph, p, seed, act if act is not False else None)
            if act is False:
                rst = self.activation(rst)
        else:
            # widths the dense kernel does not cover: the dense part in torch, dropout and aggregation on the kernels
            from .autograd import copy_reduce
            hd = _DropoutRows.apply(feat, p, seed) if p > 0 else feat
            rst = self.fc_self(hd) + self.fc_neigh(copy_reduce(graph, hd, "mean"))
            if self.activation is not None:
                rst = self.activation(rst)
        if self.norm is not None:
            rst = self.norm(rst)
        return rst

    def extra_repr(self):
        return "in=%d, out=%d, aggregator=%s, feat_drop=%s" % (self._in_feats, self._out_feats, self._aggre_type,
                                                              self.feat_drop.p)
