"""Relational graph convolution (Schlichtkrull et al., ESWC 2018) on the HIP kernels: ``RelGraphConv`` is what
``dgl.nn.pytorch.conv.RelGraphConv`` resolves to after ``compat.install_as_dgl()`` - the relation-aware baseline of a
knowledge-graph recommender.

Semantics of DGL 0.4.x ``RelGraphConv(in_feat, out_feat, num_rels, regularizer="basis", num_bases, bias, activation,
self_loop, dropout)`` with feature input:

    W_r = sum_b w_comp[r, b] * weight[b]            (W_r = weight[r] when num_bases == num_rels)
    h[v] = sum_{e: u->v} norm[e] * (x[u] @ W_{etype[e]})
    h += h_bias;  h += x @ loop_weight;  h = activation(h);  h = dropout(h)

with ``weight`` (B, in, out), ``w_comp`` (R, B) only when B < R, ``h_bias`` (out) zeros, ``loop_weight`` (in, out) only
with ``self_loop`` - the names and shapes of DGL, so a state_dict of a DGL run loads unchanged - all but the bias
xavier-uniform with the gain of relu.  The layer runs aggregate-first: ``autograd.rgcn_aggregate`` gathers every source
row once and forms Z[v, b, :] = sum norm[e] w_comp[etype[e], b] x[u, :] (kgat_rgcn_fwd_f32, with its two backward
walks), then ``h = Z.view(N, B * in) @ weight.view(B * in, out)`` is a torch matmul under torch's autograd.  With
B == R the coefficients are the R x R identity, a constant.  The dropout is this package's counter-hash mask over the
output: ``ops.dropout_keep_mask(seed, N, out_feat, p)``."""
import torch
import torch.nn as nn

from ._lib import KGATLibraryError
from .sage_layer import _DropoutRows, draw_seed


class RelGraphConv(nn.Module):
    """dgl.nn.pytorch.conv.RelGraphConv (DGL 0.4.x, regularizer "basis") on the HIP kernels."""

    def __init__(self, in_feat, out_feat, num_rels, regularizer="basis", num_bases=None, bias=True, activation=None,
                 self_loop=False, dropout=0.0):
        super().__init__()
        if isinstance(in_feat, (tuple, list)):
            raise NotImplementedError("RelGraphConv: bipartite (tuple) inputs are not supported; only homogeneous graphs")
        if regularizer != "basis":
            if regularizer == "bdd":
                raise NotImplementedError("RelGraphConv: the block-diagonal decomposition (regularizer='bdd') is not "
                                          "implemented; use regularizer='basis'")
            raise ValueError('RelGraphConv: regularizer must be "basis" or "bdd", got %r' % (regularizer,))
        self.in_feat, self.out_feat, self.num_rels = in_feat, out_feat, num_rels
        self.regularizer = regularizer
        if num_bases is None or num_bases > num_rels or num_bases <= 0:
            num_bases = num_rels
        self.num_bases = num_bases
        self.bias, self.activation, self.self_loop = bias, activation, self_loop
        self.weight = nn.Parameter(torch.empty(num_bases, in_feat, out_feat))
        if num_bases < num_rels:
            self.w_comp = nn.Parameter(torch.empty(num_rels, num_bases))
        if bias:
            self.h_bias = nn.Parameter(torch.empty(out_feat))
        if self_loop:
            self.loop_weight = nn.Parameter(torch.empty(in_feat, out_feat))
        self.dropout = nn.Dropout(dropout)
        self.reset_parameters()

    def reset_parameters(self):
        gain = nn.init.calculate_gain("relu")
        nn.init.xavier_uniform_(self.weight, gain=gain)
        if self.num_bases < self.num_rels:
            nn.init.xavier_uniform_(self.w_comp, gain=gain)
        if self.bias:
            nn.init.zeros_(self.h_bias)
        if self.self_loop:
            nn.init.xavier_uniform_(self.loop_weight, gain=gain)

    def drop_p(self):
        return self.dropout.p if self.training else 0.0

    def coefficients(self):
        """(R, B): w_comp, or the R x R identity (a constant) when every relation has its own weight."""
        if self.num_bases < self.num_rels:
            return self.w_comp
        return torch.eye(self.num_rels, dtype=self.weight.dtype, device=self.weight.device)

    def forward(self, g, x, etypes, norm=None, seed=None):
        from .autograd import rgcn_aggregate
        from .graph import DGLError
        if isinstance(x, (tuple, list)):
            raise NotImplementedError("RelGraphConv: bipartite (tuple) inputs are not supported")
        if g.partition is not None:
            raise DGLError("RelGraphConv on a partitioned graph is not supported (sharded relational convolution is "
                           "out of scope)")
        if not x.is_floating_point():
            raise NotImplementedError("RelGraphConv: featureless input (integer node ids selecting rows of the weight) "
                                      "is not implemented; pass an embedding's rows")
        if x.dim() != 2 or x.shape[1] != self.in_feat:
            raise ValueError("RelGraphConv: x must be (N, %d), got %s" % (self.in_feat, tuple(x.shape)))
        if x.shape[0] != g.number_of_nodes():
            raise ValueError("node feature has %d rows, graph has %d nodes" % (x.shape[0], g.number_of_nodes()))
        if not x.is_cuda:
            raise KGATLibraryError("x is on %s: RelGraphConv only runs on a HIP device (no CPU implementation exists in "
                                   "this package)" % (x.device,))
        p = self.drop_p()
        if p > 0 and seed is None:
            seed = draw_seed()
        seed = 0 if seed is None else int(seed)
        Z = rgcn_aggregate(g, x, self.coefficients(), etypes, norm)                      # (N, B, in)
        h = Z.view(Z.shape[0], -1) @ self.weight.view(self.num_bases * self.in_feat, self.out_feat)
        if self.bias:
            h = h + self.h_bias
        if self.self_loop:
            h = h + x @ self.loop_weight
        if self.activation is not None:
            h = self.activation(h)
        if p > 0:
            h = _DropoutRows.apply(h, p, seed)
        return h

    def extra_repr(self):
        return "in=%d, out=%d, rels=%d, bases=%d, self_loop=%s, dropout=%s" % (
            self.in_feat, self.out_feat, self.num_rels, self.num_bases, self.self_loop, self.dropout.p)
