"""KGAT's attentive embedding-propagation layer on the DGLGraph surface of this package.

A from-scratch restatement of the reference's model glue for the hot path (SURVEY.md 8a rows
A1, B1, B2): ``KGATConv`` follows reference models.py:49-70, ``KGATPropagation.compute_attention``
models.py:146-154 and ``KGATPropagation.gnn`` models.py:156-168.  Parameter names and shapes
match the reference's ``Model`` (``entity_embed.weight`` (N,d), ``relation_embed.weight`` (R,k),
``W_R`` (R,d,k), ``layers.i.res_fc_2.weight`` (D_out,D_in)) so its state_dict loads unchanged.

Two ways through every step:
* the *surface* way - the very call sequence of the reference (``filter_edges`` /
  ``apply_edges`` per relation, ``edge_softmax``, ``update_all``), exercising the drop-in
  boundary; and
* the *fused* way - ``g.kgat_attention`` (one attention launch over relation-grouped edges)
  and the SpMM with the ``h * h_N`` product in its epilogue.  Same results, fewer passes.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import function as fn
from .autograd import _combine, edge_softmax, u_mul_e_sum
from .ckg_io import load_pretrained_rows
from .kg_eval import LinkPrediction
from .ops import BI2_FORM, FORMS
from .options import options
from .rgcn_layer import RelGraphConv
from .sage_layer import SAGEConv, draw_seed


def _i32(ts):
    """Id tensors as the kernels take them: contiguous int32 ones are used as they are."""
    return [t if t.dtype == torch.int32 and t.is_contiguous() else t.to(torch.int32).contiguous() for t in ts]


# what KGATConv's res_type may be -> the form ops.aggregator* take: the ops.FORMS values and the two-term Bi-Interaction
RES_TYPES = dict(FORMS, Bi2=BI2_FORM)


def _layer_dense(layer):
    """(form, weight, d_in, d_out) of a KGAT layer's dense part: RES_TYPES[res_type] and res_fc_2 / res_fc (a
    reference-shaped layer routed here by compat.accelerate has res_fc_2 and no _res_type: Bi).  A two-term layer
    ("Bi2") has both linears: its weight is the pair (res_fc.weight, res_fc_2.weight)."""
    if getattr(layer, "_res_type", None) == "Bi2":
        lin = layer.res_fc
        return BI2_FORM, (lin.weight, layer.res_fc_2.weight), lin.in_features, lin.out_features
    if hasattr(layer, "res_fc_2"):
        lin = layer.res_fc_2
        return FORMS["Bi"], lin.weight, lin.in_features, lin.out_features
    form, lin = FORMS[layer._res_type], layer.res_fc
    return form, lin.weight, lin.in_features // (2 if form == FORMS["GraphSage"] else 1), lin.out_features


def _raw(W):
    """A layer's weight as the kernels take it, detached and contiguous: a tensor, or the two-term layer's pair."""
    return tuple(_raw(w) for w in W) if isinstance(W, tuple) else W.detach().contiguous()


def ops_transr_supported(model, h):
    from . import ops
    n_rel, d, k = model.W_R.shape
    return ops.transr_supported(model.entity_embed.weight.shape[0], d, k, n_rel, h.numel())


class _TallLinear(torch.autograd.Function):
    """``x @ W^T`` for a tall x (N ~ 10^5 rows, <= 128 columns).  Forward and grad_x are ordinary
    library GEMMs; the weight gradient ``grad^T @ x`` reduces over N into a tiny (D_out, D_in)
    result, a shape the library handles badly (0.45-0.5 ms at N = 159k against ~25 us for the
    other two GEMMs), so it is computed as a batched GEMM over row slabs plus a sum."""

    SLABS = 128

    @staticmethod
    def forward(ctx, x, weight):
        ctx.save_for_backward(x, weight)
        return F.linear(x, weight)

    @staticmethod
    def backward(ctx, grad):
        x, weight = ctx.saved_tensors
        grad = grad.contiguous()
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = grad @ weight
        if ctx.needs_input_grad[1]:
            from .autograd import tall_weight_grad
            gw = tall_weight_grad(grad, x, _TallLinear.SLABS)
        return gx, gw


class KGATConv(nn.Module):
    """KGAT propagation layer (reference models.py:49-70), then dropout, with one of the KGAT paper's aggregators
    ("Information Aggregation"; the reference implements only ``Bi`` and keeps ``res_type`` as the hook):
      * ``"Bi"``        LeakyReLU_{0.01}(res_fc_2(h * h_N))       res_fc_2.weight (out, in)
      * ``"GCN"``       LeakyReLU_{0.01}(res_fc(h + h_N))         res_fc.weight (out, in)
      * ``"GraphSage"`` LeakyReLU_{0.01}(res_fc([h | h_N]))       res_fc.weight (out, 2 in): columns [:in] act on h
      * ``"Bi2"``       LeakyReLU_{0.01}(res_fc(h + h_N)) + LeakyReLU_{0.01}(res_fc_2(h * h_N)): the paper's two-term
                        Bi-Interaction (eq. 8), both weights (out, in); the reference's ``Bi`` is its second term."""

    def __init__(self, entity_in_feats, out_feats, dropout, res_type="Bi"):
        super().__init__()
        if res_type not in RES_TYPES:
            raise NotImplementedError(res_type)
        self.mess_drop = nn.Dropout(dropout)
        self._res_type = res_type
        if res_type == "Bi2":  # (the reference's own names: res_fc on the sum - models.py:55 - res_fc_2 on the product)
            self.res_fc = nn.Linear(entity_in_feats, out_feats, bias=False)
            self.res_fc_2 = nn.Linear(entity_in_feats, out_feats, bias=False)
        elif res_type == "Bi":
            self.res_fc_2 = nn.Linear(entity_in_feats, out_feats, bias=False)
        else:
            k = 2 * entity_in_feats if res_type == "GraphSage" else entity_in_feats
            self.res_fc = nn.Linear(k, out_feats, bias=False)

    def _dense(self, h, h_neighbor, fused):
        """The GCN / GraphSage / Bi2 dense part: LeakyReLU(res_fc(h + h_N | [h | h_N])), for Bi2 plus
        LeakyReLU(res_fc_2(h * h_N)).  fused and nothing to differentiate: the aggregator kernel (ops.aggregator) where
        it covers the widths; otherwise library GEMMs."""
        from . import ops
        form, W, d_in, d_out = _layer_dense(self)
        ws = W if isinstance(W, tuple) else (W,)
        if (fused and h.is_cuda and h.dtype == torch.float32 and ops.aggregator_supported(form, d_in, d_out) and
                not (torch.is_grad_enabled() and any(x.requires_grad for x in (h, h_neighbor, *ws)))):
            return ops.aggregator(form, h.contiguous(), h_neighbor.contiguous(), _raw(W), 0.01)
        terms = [F.leaky_relu(_TallLinear.apply(x, w)) for x, w in zip(_combine(form, h, h_neighbor), ws)]
        return terms[0] if len(terms) == 1 else terms[0] + terms[1]

    def forward(self, g, nfeat, fused=None, seed=None):
        part = g.partition
        if fused is None:
            fused = not (torch.is_grad_enabled() and nfeat.requires_grad)
        if part is not None:
            if self._res_type != "Bi":
                from .graph import DGLError
                raise DGLError("KGATConv(res_type=%r) on a partitioned graph: sharded models run the Bi aggregator only"
                               % (self._res_type,))
            if torch.is_grad_enabled() and (nfeat.requires_grad or self.res_fc_2.weight.requires_grad):
                # differentiable shard layer (partition._ShardConv): local backward + all-reduce of the
                # gradients of the replicated operands; dropout is its hash mask, drawn on global rows
                from . import ops
                from .graph import DGLError
                from .partition import shard_conv
                # the shard layer treats the edge weights as constants (kgat.py:142-144 computes them under
                # no_grad) and runs the fused bi-interaction kernels: refuse what it cannot differentiate
                # instead of dropping a gradient or failing inside autograd
                if g.edata["w"].requires_grad:
                    raise DGLError("KGATConv on a shard does not differentiate through the edge weights "
                                   "(g.edata['w'].requires_grad is True): detach them, or use the unsharded graph")
                lin = self.res_fc_2
                if not ops.bi_interaction_supported(lin.in_features, lin.out_features):
                    raise DGLError("KGATConv on a shard under autograd supports the bi-interaction kernel's widths "
                                   "only; got %d -> %d" % (lin.in_features, lin.out_features))
                p = self.mess_drop.p if self.training else 0.0
                if seed is None:
                    seed = int(torch.empty((), dtype=torch.int64).random_()) if p > 0 else 0
                return shard_conv(part, g, nfeat, self.res_fc_2.weight, 0.01, p, seed)
            out = part.propagate(g, nfeat, self.res_fc_2.weight)
        elif fused and self._res_type != "Bi":
            out = self._dense(nfeat, u_mul_e_sum(g, nfeat, g.edata["w"]), fused=True)
        elif fused:
            # h * h_N formed in the SpMM epilogue (models.py:63 + the th.mul of :66)
            prod = u_mul_e_sum(g, nfeat, g.edata["w"], mul_self=True)
            out = F.leaky_relu(self.res_fc_2(prod))
        else:
            g = g.local_var()
            g.ndata["h"] = nfeat
            g.update_all(fn.u_mul_e("h", "w", "m"), fn.sum("m", "h_neighbor"))
            h_neighbor = g.ndata["h_neighbor"]
            if self._res_type != "Bi":
                out = self._dense(g.ndata["h"], h_neighbor, fused=False)
            else:
                out = F.leaky_relu(_TallLinear.apply(torch.mul(g.ndata["h"], h_neighbor), self.res_fc_2.weight))
        return self.mess_drop(out)


class KGATPropagation(LinkPrediction, nn.Module):
    """The hot-path part of the reference's ``Model`` (models.py:72-111,135-168): embeddings,
    W_R, the KGATConv stack, ``compute_attention`` and ``gnn``.  The TransR / BPR losses of the
    reference (models.py:114-133,170-178) are outside this path; ``get_loss`` is kept because the
    training-step test needs a scalar to differentiate.

    ``use_attention=False`` (reference kgat.py:27, models.py:73; the paper's "w/o Att"): ``compute_attention`` returns
    the Laplacian weights ``g.laplacian_weights(adj_type)`` (kgat.py:19: "si" D^-1 A, "bi" D^-1/2 A D^-1/2) instead of
    the attention - the epoch loop needs no other change.  ``node_dropout`` (the paper's second regulariser): in
    training mode with gradients enabled every ``gnn`` call drops each edge with that probability and scales the
    survivors by 1 / (1 - p); one dropped adjacency per call, shared by all layers and by the backward.  The three
    add no parameter or buffer.

    ``gnn_model="rgcn"`` (``num_bases``): a stack of ``RelGraphConv`` layers with ``min(num_bases, n_relations)`` bases
    and a self-loop over the edges' types, normalised by 1 / in-degree; ``gnn`` runs it per layer (``_gnn_rgcn``), the
    edge weights in ``edata['w']`` are not read.

    Draw order of a ``gnn`` call (torch's CPU generator, so ``torch.manual_seed`` reproduces a run): first the
    message-dropout seed - one ``torch.empty((), dtype=torch.int64).random_()``, drawn only by the fused training unit
    and only when the layers' dropout is > 0 -, then the node-dropout seed - one more such draw, only when node dropout
    applies.  The edges kept are ``ops.edge_keep_mask(seed, E, node_dropout)``, by edge id."""

    def __init__(self, n_entities, n_relations, input_node_dim=64, relation_dim=64, num_gnn_layers=3,
                 n_hidden=64, dropout=0.1, reg_lambda_gnn=0.01, gnn_model="kgat", res_type="Bi", use_attention=True,
                 adj_type="si", node_dropout=0.0, num_bases=4):
        super().__init__()
        if gnn_model not in ("kgat", "graphsage", "rgcn"):
            raise NotImplementedError("gnn_model must be 'kgat', 'graphsage' or 'rgcn', got %r" % (gnn_model,))
        if res_type not in RES_TYPES:
            raise NotImplementedError("res_type must be one of %s, got %r" % (", ".join(sorted(RES_TYPES)), res_type))
        if gnn_model in ("graphsage", "rgcn") and res_type != "Bi":
            raise ValueError("res_type selects the aggregator of gnn_model='kgat'; gnn_model=%r takes none "
                             "(got res_type=%r)" % (gnn_model, res_type))
        if adj_type not in ("si", "bi"):
            raise ValueError("adj_type must be 'si' or 'bi', got %r" % (adj_type,))
        if not 0.0 <= float(node_dropout) < 1.0:
            raise ValueError("node_dropout must be in [0, 1), got %r" % (node_dropout,))
        if gnn_model == "graphsage" and node_dropout > 0:
            raise ValueError("node_dropout scales the edge weights; gnn_model='graphsage' aggregates without weights "
                             "(got node_dropout=%r)" % (node_dropout,))
        if gnn_model == "rgcn" and node_dropout > 0:
            raise ValueError("node_dropout scales the attention's edge weights; gnn_model='rgcn' aggregates with the "
                             "Laplacian normaliser (got node_dropout=%r)" % (node_dropout,))
        if gnn_model == "rgcn" and int(num_bases) < 1:
            raise ValueError("num_bases must be at least 1, got %r" % (num_bases,))
        self._gnn_model = gnn_model
        self._res_type = res_type
        self._use_attention, self._adj_type, self._node_dropout = bool(use_attention), adj_type, float(node_dropout)
        self._n_entities, self._n_relations = n_entities, n_relations
        self._reg_lambda_gnn = reg_lambda_gnn
        self.entity_embed = nn.Embedding(n_entities, input_node_dim)
        self.relation_embed = nn.Embedding(n_relations, relation_dim)
        self.W_R = nn.Parameter(torch.empty(n_relations, input_node_dim, relation_dim))
        nn.init.xavier_uniform_(self.W_R, gain=nn.init.calculate_gain("relu"))
        self.layers = nn.ModuleList()
        for i in range(num_gnn_layers):  # widths: models.py:91-111
            d_in = input_node_dim if i == 0 else n_hidden // int(math.pow(2, i - 1))
            if gnn_model == "graphsage":  # models.py:98-100,107-109: ReLU on every layer but the last
                act = None if i + 1 == num_gnn_layers else F.relu
                self.layers.append(SAGEConv(d_in, n_hidden // int(math.pow(2, i)), aggregator_type="mean",
                                            feat_drop=dropout, activation=act))
            elif gnn_model == "rgcn":  # R-GCN with basis decomposition; ReLU on every layer but the last
                act = None if i + 1 == num_gnn_layers else F.relu
                self.layers.append(RelGraphConv(d_in, n_hidden // int(math.pow(2, i)), n_relations,
                                                num_bases=min(int(num_bases), n_relations), self_loop=True,
                                                dropout=dropout, activation=act))
            else:
                self.layers.append(KGATConv(d_in, n_hidden // int(math.pow(2, i)), dropout, res_type))

    # -- attention (models.py:135-154)
    def _att_score(self, edges):
        t_r = torch.matmul(self.entity_embed(edges.src["id"]), self.W_r)
        h_r = torch.matmul(self.entity_embed(edges.dst["id"]), self.W_r)
        # the batched dot product of models.py:143 (a bmm of (B,1,k) x (B,k,1) there: 1.5 ms per relation in the
        # library's batched GEMM on this shape, 61 of the surface's 72 ms - profiles/r05_surface_trace_summary.txt)
        att_w = (t_r * torch.tanh(h_r + self.relation_embed(edges.data["type"]))).sum(-1, keepdim=True)
        return {"att_w": att_w}

    def compute_attention_surface(self, g):
        """The reference's own call sequence over the drop-in surface."""
        g = g.local_var()
        for i in range(self._n_relations):
            e_idxs = g.filter_edges(lambda edges: edges.data["type"] == i)
            self.W_r = self.W_R[i]
            g.apply_edges(self._att_score, e_idxs)
        return edge_softmax(g, g.edata.pop("att_w"))

    def compute_attention(self, g, algo="auto", differentiable=False):
        """Fused: one attention-logit launch over relation-grouped edges + destination softmax.
        The kernels index the table by node position; `_node_embeddings` is the table itself when
        ndata['id'] is arange(N) (dataset.py:118) and entity_embed(ids) otherwise (models.py:140-141).
        use_attention=False: the Laplacian weights of adj_type (graph-static, cached with the graph).
        The result is a constant whatever the autograd state (kgat.py:142-144).  differentiable=True: the same values
        as a plain tensor that carries the gradient to entity_embed, W_R and relation_embed (DGLGraph.kgat_attention);
        ``gnn`` then runs its per-layer path, whose aggregation returns the weight gradient."""
        if not getattr(self, "_use_attention", True):
            if differentiable:
                raise ValueError("compute_attention(differentiable=True) with use_attention=False: the Laplacian "
                                 "weights have no parameter to differentiate towards")
            return g.laplacian_weights(self._adj_type)
        return g.kgat_attention(self._node_embeddings(g), self.W_R, self.relation_embed.weight, algo=algo,
                                differentiable=differentiable)

    def explain(self, g, users, items, max_len=None, top=1):
        """The highest-attention walks from items[q] to users[q] under the edge weights in ``g.edata['w']``
        (explain.attention_paths; the case study of the KGAT paper, section 4.5).  max_len defaults to the number of
        propagation layers: the walks the stack can carry information along.  top in 2..4: that many ranked walks per
        length (a ``TopAttentionPaths``)."""
        from .explain import attention_paths
        return attention_paths(g, g.edata["w"], users, items, max_len=len(self.layers) if max_len is None else max_len,
                               top=top)

    # -- propagation (models.py:156-168)
    def gnn(self, g, x=None, fused=None):
        if self._sage_stack():
            return self._gnn_sage(g, fused)
        if len(self.layers) > 0 and all(isinstance(layer, RelGraphConv) for layer in self.layers):
            return KGATPropagation._gnn_rgcn(self, g)  # (not through self: a model routed here by compat.accelerate lacks it)
        if g.partition is not None and any(_layer_dense(layer)[0] != FORMS["Bi"] for layer in self.layers):
            from .graph import DGLError
            raise DGLError("res_type %r on a partitioned graph: sharded models run the Bi aggregator only"
                           % (self._res_type,))
        auto = fused is None
        if auto:
            fused = not torch.is_grad_enabled()
        # node dropout: training mode under autograd only (a reference-shaped model routed here has none)
        edge_p = getattr(self, "_node_dropout", 0.0) if (self.training and torch.is_grad_enabled()) else 0.0
        if edge_p > 0:
            from .graph import DGLError
            if g.partition is not None:
                raise DGLError("node_dropout on a partitioned graph is not supported: it runs on one GPU")
            if g.edata["w"].requires_grad:
                raise DGLError("node_dropout treats the edge weights as constants (kgat.py:139-145 computes them "
                               "under no_grad): g.edata['w'].requires_grad is True")
        if edge_p == 0 and fused and self._can_fuse_readout():
            return self._gnn_fused(g) if g.partition is None else self._gnn_fused_sharded(g)
        if auto and self._can_fuse_training(g):
            # training mode (kgat.py:146-168): the whole stack as one autograd unit; the dropout mask
            # seed comes from torch's CPU generator, so torch.manual_seed reproduces a run
            from .autograd import gnn_train
            p = self.layers[0].mess_drop.p if self.training else 0.0
            seed = int(torch.empty((), dtype=torch.int64).random_()) if p > 0 else 0
            edge_seed = int(torch.empty((), dtype=torch.int64).random_()) if edge_p > 0 else 0
            dense = [_layer_dense(layer) for layer in self.layers]
            # (a two-term layer's d[1] is its pair of weights)
            return gnn_train(g, self._node_embeddings(g), [d[1] for d in dense], 0.01, p, seed,
                             forms=[d[0] for d in dense], edge_drop_p=edge_p, edge_seed=edge_seed)
        if auto and g.partition is not None and torch.is_grad_enabled() and self._can_fuse_training(g, sharded=True):
            return self._gnn_train_sharded(g)
        g = g.local_var()
        if edge_p > 0:
            g.edata["w"] = self._dropped_edge_weights(g, edge_p, int(torch.empty((), dtype=torch.int64).random_()))
        h = self._node_embeddings(g)
        node_embed_cache = [h]
        for layer in self.layers:
            # (a reference-shaped model routed here by compat.accelerate has the reference's own layers)
            h = layer(g, h, fused=fused) if isinstance(layer, KGATConv) else layer(g, h)
            node_embed_cache.append(F.normalize(h, p=2, dim=1))
        return torch.cat(node_embed_cache, 1)

    @staticmethod
    def _dropped_edge_weights(g, p, seed):
        """The per-layer path's node dropout: the dropped weights in edge-id order for the local_var graph's
        edata['w'], with their CSR-order stream (and, on first use in backward, the reversed one) kept beside them in
        the structure's slot for dropped weights - the layers' aggregations take those, permute nothing and leave the
        cached copies of the undropped weights alone."""
        from . import ops
        st = g._st
        w = g.edata["w"]
        flat = st._flat(w).detach().contiguous()
        csr = st.csr(flat.device)
        w_csr = ops.edge_dropout(st.csr_weights(w), csr.eid, p, seed)
        dropped = ops.edge_dropout(flat, None, p, seed)

        def make_rev():
            return ops.edge_dropout(st.rev_weights(w), st.csr_rev(flat.device).eid, p, seed)
        st.remember_dropped(dropped, w_csr, make_rev)
        return dropped.reshape(w.shape)

    def _gnn_train_sharded(self, g):
        """Training mode on a destination-range shard (kgat.py:146-168 on N GPUs): every layer is a
        differentiable shard layer (partition.shard_conv), the readout is assembled from the
        exchanged layer outputs on every rank.  The dropout seed is drawn as the unsharded training
        path draws it (one draw from torch's CPU generator per call, layer i uses seed + i), and the
        hash mask is indexed by global row: with the same torch.manual_seed the shards reproduce the
        one-GPU run's masks."""
        from .partition import shard_conv
        p = self.layers[0].mess_drop.p if self.training else 0.0
        seed = int(torch.empty((), dtype=torch.int64).random_()) if p > 0 else 0
        h = self._node_embeddings(g)
        cache = [h]
        for li, layer in enumerate(self.layers):
            # (the gradient of a layer's input is needed in full only where that input is a replicated parameter -
            # the embedding table under layer 0; deeper layers reduce it to the rows' owners)
            h = shard_conv(g.partition, g, h, layer.res_fc_2.weight, 0.01, p, seed + li,
                           owner_only_grad=li > 0)
            cache.append(F.normalize(h, p=2, dim=1))
        return torch.cat(cache, 1)

    def _can_fuse_training(self, g, sharded=False):
        from . import ops
        if not all(isinstance(layer, KGATConv) or hasattr(layer, "res_fc_2") for layer in self.layers):
            return False
        w = self.entity_embed.weight
        dense = [_layer_dense(layer) for layer in self.layers]
        if sharded and any(d[0] != FORMS["Bi"] for d in dense):
            return False
        return ((g.partition is None) != sharded and w.is_cuda and w.dtype == torch.float32 and "w" in g.edata and
                not g.edata["w"].requires_grad and
                all(ops.aggregator_supported(form, d_in, d_out) and layer.mess_drop.p < 1.0
                    for layer, (form, _, d_in, d_out) in zip(self.layers, dense)))

    def _node_embeddings(self, g):
        """entity_embed(g.ndata['id']) (models.py:159); the reference's ids are arange(N)
        (dataset.py:118), in which case the lookup is the table itself."""
        ids = g.ndata["id"]
        # cached on the tensor object itself (held here, so its identity cannot be recycled by the
        # allocator for another graph's ids) and its version counter
        hit = getattr(self, "_ids_hit", None)
        if hit is None or hit[0] is not ids or hit[1] != ids._version:
            same = (ids.numel() == self._n_entities and
                    bool(torch.equal(ids, torch.arange(ids.numel(), device=ids.device, dtype=ids.dtype))))
            hit = self._ids_hit = (ids, ids._version, same)
        return self.entity_embed.weight if hit[2] else self.entity_embed(ids)

    def _can_fuse_readout(self):
        from . import ops
        if not all(isinstance(layer, KGATConv) or hasattr(layer, "res_fc_2") for layer in self.layers):
            return False
        drop_off = all((not layer.training) or layer.mess_drop.p == 0 for layer in self.layers)
        return drop_off and all(ops.aggregator_supported(form, d_in, d_out)
                                for form, _, d_in, d_out in map(_layer_dense, self.layers))

    def _gnn_fused(self, g):
        """No-grad fast path: the plain aggregation, then one kernel per layer for h * h_N (or the layer's other
        combination) + Linear + LeakyReLU + the L2-normalised copy written into its slice of the output."""
        from . import ops
        h = self._node_embeddings(g).detach()
        dense = [_layer_dense(layer) for layer in self.layers]
        widths = [h.shape[1]] + [d[3] for d in dense]
        out = torch.empty((h.shape[0], sum(widths)), dtype=torch.float32, device=h.device)
        h0 = h
        off = widths[0]
        w = g.edata["w"]
        # the first layer's dense kernel also writes the ego block (self_out: the rows of its input are in registers
        # anyway) instead of an N x d copy pass at the end: step 0.491 -> 0.481 ms on the benchmark graph
        copy_self = widths[0] % 4 == 0
        # KGAT_FUSE_BI=1: aggregation and dense part of a layer in ONE launch where the widths allow
        # (kgat_spmm_bi_fused_f32: the rows h * h_N stay with the workgroup that completed them; same bits as the
        # two launches).  Off by default: measured 3-4 % SLOWER per layer than the two launches on the benchmark
        # graph (119.7 vs 116.4 us at 64 -> 64, profiles/r04_fused_bi_ab.txt) - the dense tail
        # keeps a workgroup's gather slots idle, which costs the latency-bound aggregation more than the 82 MB
        # round trip of h * h_N costs the separate launch.
        # (it computes the product alone: a GCN / GraphSage / Bi2 layer skips it and takes its dense kernel below)
        fuse_bi = options.fuse_bi
        defer = options.gnn_defer_finish
        st = g._st
        scratch = None
        for li, (form, W, _, _) in enumerate(dense):
            last = li + 1 == len(self.layers)
            lo, off = off, off + widths[li + 1]
            norm_out = out[:, lo:off]
            self_out = out[:, :widths[0]] if (li == 0 and copy_self) else None
            hc = h.contiguous()
            if (form == FORMS["Bi"] and fuse_bi and ops.spmm_bi_fused_supported(widths[li], widths[li + 1]) and
                    lo % 4 == 0 and out.shape[1] % 4 == 0 and h.shape[0] > 0):
                csr = st.csr(h.device)
                if scratch is None or scratch.shape[1] != widths[li]:
                    # (kept with the graph's per-device structure, as the permutation's scratch is: the launches of one
                    # stream share it, and a step allocates nothing for it)
                    cache, key = st._cache(h.device), ("bi_scratch", h.shape[0], widths[li])
                    scratch = cache.get(key)
                    if scratch is None:
                        scratch = cache[key] = ops._scratch((h.shape[0], widths[li]), torch.float32, h.device)
                h = ops.spmm_bi_fused(csr.indptr, csr.col, csr.row_of, hc, st.csr_weights(w), W.detach(), 0.01,
                                      norm_out=norm_out, want_h=not last, scratch=scratch, self_out=self_out)
                continue
            # the plain aggregation; h * h_N is formed by the dense kernel while it loads its rows (as an epilogue of
            # the aggregation it is a dependent X[v] load per finished row inside the edge loop: 91 vs 78 us per
            # launch).  The aggregation's second launch (the sums of the rows its edge tiles cut, the zero rows) is
            # left to the dense kernel too: it forms those rows from the tiles' partials in the same order of
            # additions (KGAT_SPMM_DEFER_FINISH; same bits, one dependent launch less per layer: step 0.4415 ->
            # 0.43 ms).  KGAT_GNN_DEFER_FINISH=0 restores the two launches.
            if defer and ops.bi_interaction_deferral_supported(widths[li], widths[li + 1]) and h.shape[0] > 0:
                csr = st.csr(h.device)
                hn, rows_left = ops.spmm(csr.indptr, csr.col, csr.row_of, hc, st.csr_weights(w), defer_finish=True)
            else:
                hn, rows_left = u_mul_e_sum(g, h, w), None
            h = ops.aggregator(form, hc, hn, _raw(W), 0.01, norm_out=norm_out, want_h=not last, deferred=rows_left,
                               self_out=self_out)
        # the ego-embedding block last: the pass ends having just touched the embedding table, which
        # is what the next attention refresh gathers from (a step's working set is about the size
        # of the 256 MiB Infinity Cache; written first, the table was the oldest resident by then:
        # the attention launch measured 0.231 ms inside the step against 0.19 ms on its own)
        if not copy_self:
            out[:, :widths[0]] = h0
        return out

    # -- GraphSAGE stack (gnn_model="graphsage", models.py:98-100,107-109; the same readout, models.py:156-168)
    def _sage_stack(self):
        return len(self.layers) > 0 and all(isinstance(layer, SAGEConv) for layer in self.layers)

    def _can_fuse_sage_readout(self):
        from . import ops
        w = self.entity_embed.weight
        return (w.is_cuda and w.dtype == torch.float32 and
                all(layer.drop_p() == 0 and layer.norm is None and layer.fused_activation() is not False and
                    ops.sage_dense_supported(layer._in_feats, layer._out_feats) and
                    layer.fc_self.bias is not None and layer.fc_neigh.bias is not None for layer in self.layers))

    def _gnn_sage(self, g, fused=None):
        """The readout [h0 | normalize(h1) | ...] over a SAGEConv stack.  No-grad (fused=None outside autograd): one
        aggregation + one dense launch per layer, the dense kernel writing its normalised slice of the readout (and,
        in layer 0, the ego block).  Otherwise the layers' autograd functions with torch's normalize / cat; the
        dropout seed is one draw from torch's CPU generator per call, layer i uses seed + i."""
        from .graph import DGLError
        if g.partition is not None:
            raise DGLError("GraphSAGE on a partitioned graph is not supported (sharded GraphSAGE is out of scope)")
        if fused is None:
            fused = not torch.is_grad_enabled()
        if fused and self._can_fuse_sage_readout():
            return self._gnn_sage_fused(g)
        seed = draw_seed() if any(layer.drop_p() > 0 for layer in self.layers) else 0
        h = self._node_embeddings(g)
        cache = [h]
        for li, layer in enumerate(self.layers):
            h = layer(g, h, seed=seed + li)
            cache.append(F.normalize(h, p=2, dim=1))
        return torch.cat(cache, 1)

    def _gnn_sage_fused(self, g):
        from . import ops
        h = self._node_embeddings(g).detach().contiguous()
        widths = [h.shape[1]] + [layer._out_feats for layer in self.layers]
        out = torch.empty((h.shape[0], sum(widths)), dtype=torch.float32, device=h.device)
        aligned = widths[0] % 4 == 0 and out.shape[1] % 4 == 0
        csr = g._st.csr(h.device)
        off = widths[0]
        for li, layer in enumerate(self.layers):
            last = li + 1 == len(self.layers)
            hn = ops.copy_reduce(csr.indptr, csr.col, csr.row_of, h, "mean")
            h = ops.sage_dense(h, hn, layer.fc_self.weight.detach(), layer.fc_neigh.weight.detach(),
                               layer.fc_self.bias.detach(), layer.fc_neigh.bias.detach(), layer.fused_activation(),
                               want_h=not last, norm_out=out[:, off:off + widths[li + 1]],
                               self_out=out[:, :widths[0]] if (li == 0 and aligned) else None)
            off += widths[li + 1]
        if not aligned:
            out[:, :widths[0]] = self._node_embeddings(g).detach()
        return out

    # -- R-GCN stack (gnn_model="rgcn": RelGraphConv layers over the typed edges; the same readout, models.py:156-168)
    def _rgcn_stack(self):
        return len(self.layers) > 0 and all(isinstance(layer, RelGraphConv) for layer in self.layers)

    def _gnn_rgcn(self, g):
        """The readout [h0 | normalize(h1) | ...] over a RelGraphConv stack, per layer: the relation of an edge is
        g.edata['type'], the normaliser the random-walk Laplacian's 1 / in-degree (g.laplacian_weights("si"), what DGL's
        R-GCN link-prediction example uses).  The dropout seed is one draw from torch's CPU generator per call, layer i
        uses seed + i."""
        from .graph import DGLError
        if g.partition is not None:
            raise DGLError("R-GCN on a partitioned graph is not supported (sharded relational convolution is out of scope)")
        etypes = g.edata["type"]
        norm = g.laplacian_weights("si")
        seed = draw_seed() if any(layer.drop_p() > 0 for layer in self.layers) else 0
        h = self._node_embeddings(g)
        cache = [h]
        for li, layer in enumerate(self.layers):
            h = layer(g, h, etypes, norm, seed=seed + li)
            cache.append(F.normalize(h, p=2, dim=1))
        return torch.cat(cache, 1)

    def transR(self, h, r, pos_t, neg_t, reg_lambda_kg=0.01, fused=None):
        """TransR pairwise ranking loss of the KG phase (reference models.py:114-133 with
        bmm_maybe_select :13-47).  On the GPU in fp32 it runs as the fused
        loss+gradient kernels (kgat_transr_loss_grad_f32, ~1,800 of these steps per amazon-book
        epoch); fused=False (and CPU / float64 modules, batches beyond the kernels' limits) takes
        the torch restatement below, which is what the parity tests compare the kernels with."""
        if fused is None:
            fused = self.entity_embed.weight.is_cuda and self.entity_embed.weight.dtype == torch.float32 and \
                ops_transr_supported(self, h)
        if fused:
            from .autograd import transr_loss
            return transr_loss(self.entity_embed.weight, self.W_R, self.relation_embed.weight, h, r, pos_t, neg_t,
                               reg_lambda_kg)
        W = self.W_R.index_select(0, r)  # (B, d, k)

        def proj(ids):
            return F.normalize(torch.bmm(self.entity_embed(ids).unsqueeze(1), W).squeeze(1), p=2, dim=1)

        h_vec, pos_vec, neg_vec = proj(h), proj(pos_t), proj(neg_t)
        r_vec = F.normalize(self.relation_embed(r), p=2, dim=1)
        pos_score = (h_vec + r_vec - pos_vec).pow(2).sum(1, keepdim=True)
        neg_score = (h_vec + r_vec - neg_vec).pow(2).sum(1, keepdim=True)
        loss = (-F.logsigmoid(neg_score - pos_score)).mean()
        reg = sum((v.pow(2).sum(1) / 2.0).mean() for v in (h_vec, r_vec, pos_vec, neg_vec))
        return loss + reg_lambda_kg * reg

    def kg_step(self, h, r, pos_t, neg_t, optimizer, reg_lambda_kg=0.01):
        """One iteration of the KG phase (reference kgat.py:116-136: transR -> backward -> optimizer.step ->
        zero_grad) without the autograd bookkeeping around it: kgat_transr_loss_grad_f32 writes the loss and the three
        dense gradients into buffers kept with the model, they become the parameters' ``.grad``, ``optimizer.step()``
        runs (any torch optimiser; FusedAdam makes the whole iteration two library calls), the gradients are dropped.
        The same kernels on the same data as ``transR(...).backward()``: the same bits.  int32 index tensors are used
        as they are.  Returns the loss (a 0-dim device tensor; reading it synchronises, as loss.item() does).
        NOTE: like the reference's step - which ends in optimizer.zero_grad() - this leaves EVERY parameter's ``.grad``
        None, including gradients another phase accumulated and has not applied yet: call it between complete steps."""
        from . import ops
        ent, W_R, rel = self.entity_embed.weight, self.W_R, self.relation_embed.weight
        if not (ent.is_cuda and ent.dtype == torch.float32 and ops_transr_supported(self, h)):
            loss = self.transR(h, r, pos_t, neg_t, reg_lambda_kg)
            loss.backward()
            optimizer.step()
            optimizer.zero_grad()
            return loss.detach()
        ids = _i32((h, r, pos_t, neg_t))
        buf = getattr(self, "_kg_buffers", None)
        if buf is None or buf[1].shape != ent.shape or buf[1].device != ent.device:
            buf = self._kg_buffers = [torch.empty((), dtype=torch.float32, device=ent.device), torch.empty_like(ent),
                                      torch.empty_like(W_R), torch.empty_like(rel), None, -1]
        if buf[4] is None or buf[5] != ids[0].numel():
            buf[4:] = [ops.transr_workspace(ids[0].numel(), W_R.shape[1], W_R.shape[2], W_R.shape[0], ent.device),
                       ids[0].numel()]
        with torch.no_grad():
            out = ops.transr_loss_grad(*ids, ent.detach(), W_R.detach(), rel.detach(), reg_lambda_kg, out=buf[:4],
                                       workspace=buf[4])
        ent.grad, W_R.grad, rel.grad = buf[1], buf[2], buf[3]
        for p_ in self.parameters():       # (parameters the KG loss does not reach have no gradient in this phase)
            if p_ is not ent and p_ is not W_R and p_ is not rel:
                p_.grad = None
        optimizer.step()
        ent.grad = W_R.grad = rel.grad = None
        return out[0]

    def kg_phase(self, h, r, pos_t, neg_t, optimizer, reg_lambda_kg=0.01):
        """The KG phase of an epoch (reference kgat.py:116-136) over batches drawn up front: h, r, pos_t, neg_t are
        (n_iterations, batch) id tensors; iteration i is transR(h[i], ...) -> backward -> optimizer.step -> zero_grad.
        Returns the n_iterations losses as a device tensor (no host round trip per iteration; the reference reads
        loss.item() every step).

        With ``FusedAdam`` on the GPU: one launch sorts every batch (kgat_transr_presort_f32), then an iteration is ONE
        library call of three launches (kgat_transr_adam_step_f32: per-sample kernel, weight-gradient partials +
        gradient rows + loss, Adam on ent / W_R / rel without a dense gradient) - the bits of ``kg_step`` and of the
        reference's autograd + torch.optim.Adam sequence.  Any other optimiser / size: a loop over ``kg_step``.
        As in ``kg_step``, parameters the KG loss does not reach get no update and their ``.grad`` is left alone."""
        from . import ops
        from .optim import FusedAdam, _StepRoute, _fused_phase
        ent, W_R, rel = self.entity_embed.weight, self.W_R, self.relation_embed.weight
        if h.dim() != 2 or r.shape != h.shape or pos_t.shape != h.shape or neg_t.shape != h.shape:
            raise ValueError("kg_phase: h, r, pos_t, neg_t must share one (n_iterations, batch) shape")
        n_it, b = h.shape
        hyper = optimizer.kg_state((ent, W_R, rel)) if isinstance(optimizer, FusedAdam) else None
        fused = (hyper is not None and n_it > 0 and ent.is_cuda and ent.dtype == torch.float32 and
                 ops.transr_supported(ent.shape[0], W_R.shape[1], W_R.shape[2], W_R.shape[0], b) and
                 all(t.data_ptr() % 16 == 0 for t in (ent, W_R, rel)))
        if not fused:
            if n_it == 0:
                return torch.zeros(0, dtype=torch.float32, device=ent.device)
            # (kg_step hands back its persistent loss buffer: copy it before the next iteration overwrites it)
            return torch.stack([self.kg_step(h[i], r[i], pos_t[i], neg_t[i], optimizer, reg_lambda_kg).clone() for i in range(n_it)])
        n, n_rel, d, k = ent.shape[0], *W_R.shape
        route = _StepRoute(lambda *ids: ops.transr_presort(*ids, n, n_rel), ops.transr_adam_step, ops.TransRAdamState,
                           (n, d, k, n_rel, b, str(ent.device)), "_kg_phase_state")
        return _fused_phase(self, route, (ent, W_R, rel), _i32((h, r, pos_t, neg_t)), optimizer, hyper, reg_lambda_kg)

    # -- BPR-MF pretraining (the KGAT paper initialises its runs from MF embeddings: the release's pretrain/<dataset>/mf.npz)
    def _mf_kernels_apply(self, batch):
        """The BPR kernels can run on the table itself: fp32 on the GPU, 16-byte aligned, a width they take."""
        ent = self.entity_embed.weight
        return (ent.is_cuda and ent.dtype == torch.float32 and ent.is_contiguous() and ent.shape[1] % 4 == 0 and
                ent.data_ptr() % 16 == 0 and 1 <= batch < (1 << 29))

    def mf_step(self, u, p, n, optimizer, reg_lambda=None):
        """One iteration of BPR-MF pretraining: ``get_loss(entity_embed.weight, u, p, n)`` (reference models.py:170-178 with
        the embedding table as the readout) -> backward -> optimizer.step -> zero_grad, without the autograd bookkeeping:
        on the GPU in fp32 kgat_bpr_loss_f32 + kgat_bpr_grad_f32 write the loss and the dense gradient into buffers kept
        with the model, the gradient becomes the table's ``.grad``, ``optimizer.step()`` runs (any torch optimiser), the
        gradient is dropped.  The same kernels on the same data as ``get_loss(...).backward()``: the same bits.
        ``reg_lambda=None``: the model's ``reg_lambda_gnn``.  CPU / float64 modules, a table the kernels do not take
        (width not a multiple of 4, not 16-byte aligned): the torch operators.  Returns the loss (a 0-dim device tensor).
        As ``kg_step``, this leaves EVERY parameter's ``.grad`` None: call it between complete steps."""
        from . import ops
        ent = self.entity_embed.weight
        lam = self._reg_lambda_gnn if reg_lambda is None else reg_lambda
        if u.dim() != 1 or p.shape != u.shape or n.shape != u.shape:
            raise ValueError("mf_step: u, p, n must share one (batch,) shape")
        if not self._mf_kernels_apply(u.numel()):
            keep = self._reg_lambda_gnn
            self._reg_lambda_gnn = lam
            try:   # (a GPU table the kernels refuse - unaligned, odd width - takes the torch restatement)
                loss = self.get_loss(ent, u.long(), p.long(), n.long(), fused=False if ent.is_cuda else None)
            finally:
                self._reg_lambda_gnn = keep
            loss.backward()
            optimizer.step()
            optimizer.zero_grad()
            return loss.detach()
        ids = _i32((u, p, n))
        b = ids[0].numel()
        buf = getattr(self, "_mf_buffers", None)
        if buf is None or buf[0].shape != ent.shape or buf[0].device != ent.device or buf[1] != b:
            buf = self._mf_buffers = [torch.empty_like(ent), b,
                                      (torch.empty((), dtype=torch.float32, device=ent.device),
                                       torch.empty(b, dtype=torch.float32, device=ent.device),
                                       ops._workspace(ops._lib.load().kgat_bpr_workspace_bytes(b, ent.shape[1]), ent.device))]
        with torch.no_grad():
            e = ent.detach()
            loss, coef, ws = ops.bpr_loss(e, *ids, lam, out=buf[2])
            ent.grad = ops.bpr_grad(e, *ids, coef, lam, workspace=ws, out=buf[0])
        for p_ in self.parameters():       # (parameters the MF loss does not reach have no gradient in this phase)
            if p_ is not ent:
                p_.grad = None
        optimizer.step()
        ent.grad = None
        return loss

    def mf_phase(self, u, p, n, optimizer, reg_lambda=None):
        """BPR-MF pretraining over batches drawn up front: u, p, n are (n_iterations, batch) id tensors (int64 or int32;
        contiguous int32 is used as it is); iteration i is ``mf_step(u[i], p[i], n[i])``.  Returns the n_iterations losses
        as a device tensor (no host round trip per iteration).

        With ``FusedAdam`` on the GPU, the table in fp32 and 16-byte aligned, and a size ``ops.mf_supported`` takes (width
        a multiple of 4 up to 256, 3 * batch <= 65536: batch <= 21845, which covers the authors' MF batch of 1,024 and the
        reference's CF batch of 10,240): every batch is sorted up front (kgat_mf_presort_f32: one launch up to batch 2,730,
        three beyond), then an iteration is ONE library call of three launches
        (kgat_mf_adam_step_f32: per-sample kernel, window sums into a compact buffer + row tags + loss, Adam on the table
        without a dense gradient) - the bits of ``mf_step`` and of the autograd + torch.optim.Adam sequence.  Any other
        optimiser or size loops over ``mf_step``.  Parameters the MF
        loss does not reach get no update, and on the fused route their ``.grad`` is left alone."""
        from . import ops
        from .optim import FusedAdam, _StepRoute, _fused_phase
        ent = self.entity_embed.weight
        if u.dim() != 2 or p.shape != u.shape or n.shape != u.shape:
            raise ValueError("mf_phase: u, p, n must share one (n_iterations, batch) shape")
        n_it, b = u.shape
        lam = self._reg_lambda_gnn if reg_lambda is None else reg_lambda
        fused = (n_it > 0 and isinstance(optimizer, FusedAdam) and self._mf_kernels_apply(b) and
                 ops.mf_supported(ent.shape[0], ent.shape[1], b))
        hyper = optimizer.kg_state((ent,)) if fused else None
        if hyper is None:
            if n_it == 0:
                return torch.zeros(0, dtype=torch.float32, device=ent.device)
            # (mf_step may hand back its persistent loss buffer: copy it before the next iteration overwrites it)
            return torch.stack([self.mf_step(u[i], p[i], n[i], optimizer, lam).clone() for i in range(n_it)])
        route = _StepRoute(lambda *ids: ops.mf_presort(*ids, ent.shape[0]), ops.mf_adam_step, ops.MFAdamState,
                           (ent.shape[0], ent.shape[1], b, str(ent.device)), "_mf_phase_state")
        return _fused_phase(self, route, (ent,), _i32((u, p, n)), optimizer, hyper, lam)

    def load_pretrained(self, user_embed, item_embed, n_users):
        """Initialise from BPR-MF embeddings (the layout of the KGAT release's pretrain/<dataset>/mf.npz, ckg_io.load_pretrain):
        ``user_embed`` (n_users, d) goes to rows [0, n_users) of the entity table, ``item_embed`` (n_items, d) to rows
        [n_users, n_users + n_items) - the node layout of ckg_io: users first, then the items, then the attribute entities,
        whose rows stay as they are."""
        load_pretrained_rows(self.entity_embed.weight, user_embed, item_embed, n_users)

    def pretrained_embeddings(self, n_users, n_items):
        """The user and item blocks of the entity table as float32 CPU numpy arrays (for ckg_io.save_pretrain)."""
        ent = self.entity_embed.weight.detach()
        if n_users < 0 or n_items < 0 or n_users + n_items > ent.shape[0]:
            raise ValueError("pretrained_embeddings: %d users + %d items exceed the table's %d rows" % (n_users, n_items, ent.shape[0]))
        t = ent[:n_users + n_items].to(device="cpu", dtype=torch.float32).numpy()
        return t[:n_users].copy(), t[n_users:].copy()

    def _gnn_fused_sharded(self, g):
        """No-grad path on a destination-range shard: per layer the local aggregation, the
        bi-interaction kernel on the owned rows, one all-reduce, and the row normalisation of the
        assembled layer output into its slice of the readout."""
        from . import ops
        part = g.partition
        h = self._node_embeddings(g).detach()
        widths = [h.shape[1]] + [layer.res_fc_2.out_features for layer in self.layers]
        # every layer's assembled rows stay in an exchange buffer of the partition (one per layer),
        # and the readout - ego block copied, layer blocks normalised - is written in one pass at the
        # end (one launch instead of a normalisation per layer plus the copy)
        blocks = [h]
        for li, layer in enumerate(self.layers):
            h = part.propagate_fused(g, h, layer.res_fc_2.weight, slot=li)
            blocks.append(h)
        if len(blocks) <= 8 and all(w % 4 == 0 and w <= 128 for w in widths):
            return ops.readout_concat(blocks, [False] + [True] * len(self.layers))
        out = torch.empty((h.shape[0], sum(widths)), dtype=torch.float32, device=h.device)
        off = 0
        for li, b in enumerate(blocks):
            if li == 0:
                out[:, :widths[0]] = b
            else:
                ops.l2_normalize_rows(b, out[:, off:off + widths[li]])
            off += widths[li]
        return out

    def get_loss(self, embedding, src_ids, pos_dst_ids, neg_dst_ids, fused=None):
        """BPR loss of reference models.py:170-178.  On the GPU in fp32 (readout width a multiple of 4): the fused
        loss / gradient kernels (kgat_bpr_loss_f32, kgat_bpr_grad_f32; ~15 launches forward + backward against ~75
        torch operator launches, 0.7 ms of the CF step); fused=False (and CPU / float64) takes the torch
        restatement below, which is what the parity tests compare the kernels with."""
        if fused is None:
            fused = (embedding.is_cuda and embedding.dtype == torch.float32 and embedding.dim() == 2 and
                     embedding.shape[1] % 4 == 0 and embedding.stride(1) == 1 and embedding.stride(0) % 4 == 0 and
                     src_ids.numel() > 0)
        if fused:
            from .autograd import bpr_loss
            return bpr_loss(embedding, src_ids, pos_dst_ids, neg_dst_ids, self._reg_lambda_gnn)
        # one gather of the three id lists (one dense zero-fill + one sorted scatter in backward
        # instead of three), then split: the same rows as embedding[src_ids] etc.
        b = src_ids.shape[0]
        rows = embedding[torch.cat([src_ids, pos_dst_ids, neg_dst_ids])]
        s, p, n = rows[:b], rows[b:2 * b], rows[2 * b:]
        pos = (s * p).sum(1)
        neg = (s * n).sum(1)
        cf = -F.logsigmoid(pos - neg).mean()
        reg = sum((v.pow(2).sum(1) / 2.0).mean() for v in (s, p, n))
        return cf + self._reg_lambda_gnn * reg
