"""Graph attention (Velickovic et al., ICLR 2018) on the HIP kernels: ``GATConv`` is what
``dgl.nn.pytorch.conv.GATConv`` resolves to after ``compat.install_as_dgl()`` - the attention baseline without the
knowledge graph's relations.

Semantics of DGL 0.4.x ``GATConv(in_feats, out_feats, num_heads, feat_drop, attn_drop, negative_slope, residual,
activation)`` on a homogeneous graph:

    h = feat_drop(feat);  ft = fc(h).view(N, H, F);  el = (ft * attn_l).sum(-1);  er = (ft * attn_r).sum(-1)
    a = edge_softmax(leaky_relu(el[src] + er[dst]));  rst[v] = sum_{e->v} attn_drop(a)[e] * ft[src e]
    rst += res_fc(h).view(N, H, F) if residual;  rst = activation(rst) if activation          -> (N, H, F)

with ``fc`` / ``res_fc`` ``nn.Linear(in_feats, H * F, bias=False)`` (``res_fc`` the identity when the widths agree),
``attn_l`` / ``attn_r`` (1, H, F), all xavier-normal with the gain of relu, so a state_dict of a DGL run loads
unchanged.  The dense parts are torch operators under torch's autograd; the message passing - logits, softmax, attention
dropout and the weighted sum, forward and backward - is ``autograd.gat_aggregate`` (kgat_gat_fwd_f32 /
kgat_gat_bwd_f32), which never forms the attention as an edge tensor.  Both dropouts are this package's counter-hash
masks: ``feat_drop`` draws from ``(seed, row, column)`` of the input (``ops.dropout_keep_mask(seed, N, in_feats, p)``),
``attn_drop`` from ``(seed + 1, edge id, head)`` (``ops.dropout_keep_mask(seed + 1, E, H, p)``)."""
import torch
import torch.nn as nn

from ._lib import KGATLibraryError
from .sage_layer import _DropoutRows, draw_seed


class GATConv(nn.Module):
    """dgl.nn.pytorch.conv.GATConv (DGL 0.4.x) on the HIP kernels."""

    def __init__(self, in_feats, out_feats, num_heads, feat_drop=0.0, attn_drop=0.0, negative_slope=0.2, residual=False,
                 activation=None):
        super().__init__()
        if isinstance(in_feats, (tuple, list)):
            raise NotImplementedError("GATConv: bipartite (tuple) inputs are not supported; only homogeneous graphs")
        if not 0.0 <= float(negative_slope) <= 1.0:
            raise ValueError("GATConv: negative_slope must be in [0, 1], got %r" % (negative_slope,))
        self._num_heads = num_heads
        self._in_feats = self._in_src_feats = self._in_dst_feats = in_feats
        self._out_feats = out_feats
        self.fc = nn.Linear(in_feats, out_feats * num_heads, bias=False)
        self.attn_l = nn.Parameter(torch.empty(1, num_heads, out_feats))
        self.attn_r = nn.Parameter(torch.empty(1, num_heads, out_feats))
        self.feat_drop = nn.Dropout(feat_drop)
        self.attn_drop = nn.Dropout(attn_drop)
        self.leaky_relu = nn.LeakyReLU(negative_slope)
        if residual:
            if in_feats != out_feats * num_heads:
                self.res_fc = nn.Linear(in_feats, num_heads * out_feats, bias=False)
            else:
                self.res_fc = nn.Identity()  # (DGL's own Identity module: no parameters either)
        else:
            self.register_buffer("res_fc", None)
        self.activation = activation
        self.reset_parameters()

    def reset_parameters(self):
        gain = nn.init.calculate_gain("relu")
        nn.init.xavier_normal_(self.fc.weight, gain=gain)
        nn.init.xavier_normal_(self.attn_l, gain=gain)
        nn.init.xavier_normal_(self.attn_r, gain=gain)
        if isinstance(self.res_fc, nn.Linear):
            nn.init.xavier_normal_(self.res_fc.weight, gain=gain)

    def forward(self, graph, feat, seed=None):
        from .autograd import gat_aggregate
        from .graph import DGLError
        if isinstance(feat, (tuple, list)):
            raise NotImplementedError("GATConv: bipartite (tuple) inputs are not supported")
        if graph.partition is not None:
            raise DGLError("GATConv on a partitioned graph is not supported (sharded graph attention is out of scope)")
        if feat.shape[0] != graph.number_of_nodes():
            raise ValueError("node feature has %d rows, graph has %d nodes" % (feat.shape[0], graph.number_of_nodes()))
        if not feat.is_cuda:
            raise KGATLibraryError("feat is on %s: GATConv only runs on a HIP device (no CPU implementation exists in "
                                   "this package)" % (feat.device,))
        p_feat = self.feat_drop.p if self.training else 0.0
        p_attn = self.attn_drop.p if self.training else 0.0
        if (p_feat > 0 or p_attn > 0) and seed is None:
            seed = draw_seed()
        seed = 0 if seed is None else int(seed)
        H, F = self._num_heads, self._out_feats
        h = _DropoutRows.apply(feat, p_feat, seed) if p_feat > 0 else feat
        ft = self.fc(h).view(-1, H, F)
        el = (ft * self.attn_l).sum(-1)
        er = (ft * self.attn_r).sum(-1)
        rst = gat_aggregate(graph, ft, el, er, self.leaky_relu.negative_slope, p_attn, seed + 1)
        if self.res_fc is not None:
            rst = rst + self.res_fc(h).view(-1, H, F)
        if self.activation is not None:
            rst = self.activation(rst)
        return rst

    def extra_repr(self):
        return "in=%d, out=%d, heads=%d, feat_drop=%s, attn_drop=%s, negative_slope=%s" % (
            self._in_feats, self._out_feats, self._num_heads, self.feat_drop.p, self.attn_drop.p,
            self.leaky_relu.negative_slope)
