"""The KGAT paper's "regularisation-based" baselines, on this package's kernels.

``CFKG``: a translation model without a projection (TransE) over the whole collaborative KG, interactions included;
recommendation is the ranking of ``(u, interact, ?)``.  Its objective is the reference's ``transR`` (models.py:114-133)
with the projection removed - ``transR`` with every ``W_R[r] = I`` and d = k, the constant regulariser term included -
so the samplers, ``reg_lambda`` and the evaluation carry over.  Its KG phase is its entire training: on a HIP device in
fp32 it runs on csrc/kgat_transe.hip (three launches per iteration, no dense gradient).

``CKE``: a recommender whose item vector is ``cf latent + TransR entity embedding``: the TransR part is
``KGATPropagation``'s (the same ``transR`` / ``kg_step`` / ``kg_phase`` functions), the CF part the fused BPR loss on
the readout.  Composition over existing kernels."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .ckg_io import load_pretrained_rows
from .kg_eval import LinkPrediction
from .kgat_layer import KGATPropagation, _i32


class _TransELoss(torch.autograd.Function):
    """TransE loss of a triplet batch.  Forward: the loss and the per-sample gradient rows (kgat_transe_forward_f32);
    backward: their ordered sums into the two dense gradients, which read the incoming gradient from device memory
    (kgat_transe_backward_f32)."""

    @staticmethod
    def forward(ctx, ent, rel, h, r, pos_t, neg_t, reg_lambda):
        loss, ws = ops.transe_forward(h, r, pos_t, neg_t, ent.detach(), rel.detach(), reg_lambda)
        ctx.ws, ctx.shapes = ws, (tuple(ent.shape), tuple(rel.shape))
        ctx.save_for_backward(h, r, pos_t, neg_t)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        h, r, pos_t, neg_t = ctx.saved_tensors
        g_ent, g_rel = ops.transe_backward(h, r, pos_t, neg_t, ctx.shapes, ctx.ws, grad_scale=grad_out.detach().to(torch.float32))
        need = ctx.needs_input_grad
        return g_ent if need[0] else None, g_rel if need[1] else None, None, None, None, None, None


def transe_loss(ent, rel, h, r, pos_t, neg_t, reg_lambda):
    """Differentiable fused TransE loss; index tensors of any integer dtype."""
    return _TransELoss.apply(ent, rel, *_i32((h, r, pos_t, neg_t)), float(reg_lambda))


def transe_loss_torch(ent, rel, h, r, pos_t, neg_t, reg_lambda):
    """The TransE loss in torch operators: reference models.py:114-133 without the bmm."""
    h_vec, pos_vec, neg_vec = (F.normalize(ent[i], p=2, dim=1) for i in (h, pos_t, neg_t))
    r_vec = F.normalize(rel[r], p=2, dim=1)
    pos_score = (h_vec + r_vec - pos_vec).pow(2).sum(1, keepdim=True)
    neg_score = (h_vec + r_vec - neg_vec).pow(2).sum(1, keepdim=True)
    loss = (-F.logsigmoid(neg_score - pos_score)).mean()
    reg = sum((v.pow(2).sum(1) / 2.0).mean() for v in (h_vec, r_vec, pos_vec, neg_vec))
    return loss + reg_lambda * reg


class CFKG(LinkPrediction, nn.Module):
    """TransE over the collaborative KG.  Parameters: ``entity_embed`` (n_entities x dim), ``relation_embed``
    (n_relations x dim).

    ``.grad`` after ``kg_step`` / ``kg_phase``, on every route (fused or not, any optimiser): both parameters' ``.grad``
    is None - the reference's iteration ends in ``optimizer.zero_grad()``, and the model has no parameter the loss does
    not reach.  Call them between complete steps."""

    def __init__(self, n_entities, n_relations, dim=64, reg_lambda_kg=0.01):
        super().__init__()
        self._n_entities, self._n_relations = int(n_entities), int(n_relations)
        self.reg_lambda_kg = float(reg_lambda_kg)
        self.entity_embed = nn.Embedding(n_entities, dim)
        self.relation_embed = nn.Embedding(n_relations, dim)

    def _kernels_apply(self, batch):
        ent, rel = self.entity_embed.weight, self.relation_embed.weight
        return (ent.is_cuda and ent.dtype == torch.float32 and ent.is_contiguous() and rel.is_contiguous() and
                ent.data_ptr() % 16 == 0 and rel.data_ptr() % 16 == 0 and
                ops.transe_supported(ent.shape[0], ent.shape[1], rel.shape[0], batch))

    def transE(self, h, r, pos_t, neg_t, reg_lambda_kg=None, fused=None):
        """The pairwise ranking loss of a triplet batch.  On a HIP device in fp32 at a size ``ops.transe_supported`` takes:
        an autograd Function over kgat_transe_forward_f32 / kgat_transe_backward_f32; ``fused=False`` (and CPU / float64
        modules, other sizes): the torch restatement, which is what the parity tests compare the kernels with."""
        lam = self.reg_lambda_kg if reg_lambda_kg is None else reg_lambda_kg
        if fused is None:
            fused = self._kernels_apply(h.numel())
        if fused:
            return transe_loss(self.entity_embed.weight, self.relation_embed.weight, h, r, pos_t, neg_t, lam)
        return transe_loss_torch(self.entity_embed.weight, self.relation_embed.weight, h.long(), r.long(), pos_t.long(),
                                 neg_t.long(), lam)

    def kg_step(self, h, r, pos_t, neg_t, optimizer, reg_lambda_kg=None):
        """One iteration (reference kgat.py:116-136: loss -> backward -> optimizer.step -> zero_grad) without the autograd
        bookkeeping: kgat_transe_loss_grad_f32 writes the loss and the two dense gradients into buffers kept with the
        model, they become the parameters' ``.grad``, ``optimizer.step()`` runs (any torch optimiser), the gradients are
        dropped.  The same kernels on the same data as ``transE(...).backward()``: the same bits.  Returns the loss (a
        0-dim device tensor)."""
        ent, rel = self.entity_embed.weight, self.relation_embed.weight
        lam = self.reg_lambda_kg if reg_lambda_kg is None else reg_lambda_kg
        if not self._kernels_apply(h.numel()):
            loss = self.transE(h, r, pos_t, neg_t, lam, fused=False)
            loss.backward()
            optimizer.step()
            ent.grad = rel.grad = None
            return loss.detach()
        ids = _i32((h, r, pos_t, neg_t))
        b = ids[0].numel()
        buf = getattr(self, "_kg_buffers", None)
        if buf is None or buf[1].shape != ent.shape or buf[1].device != ent.device or buf[4] != b:
            buf = self._kg_buffers = [torch.empty((), dtype=torch.float32, device=ent.device), torch.empty_like(ent),
                                      torch.empty_like(rel), ops.transe_scratch(b, ent.shape[1], rel.shape[0], ent.device), b]
        with torch.no_grad():
            out = ops.transe_loss_grad(*ids, ent.detach(), rel.detach(), lam, out=buf[:3], scratch=buf[3])
        ent.grad, rel.grad = buf[1], buf[2]
        optimizer.step()
        ent.grad = rel.grad = None
        return out[0]

    def kg_phase(self, h, r, pos_t, neg_t, optimizer, reg_lambda_kg=None):
        """The KG phase over batches drawn up front: h, r, pos_t, neg_t are (n_iterations, batch) id tensors; iteration i
        is ``kg_step(h[i], ...)``.  Returns the n_iterations losses as a device tensor (no host round trip per iteration).

        With ``FusedAdam`` on the GPU at a size ``ops.transe_supported`` takes: one launch sorts every batch
        (kgat_transe_presort_f32), then an iteration is ONE library call of three launches (kgat_transe_adam_step_f32:
        per-sample kernel + row tags, chunk sums + loss, Adam on ent / rel without a dense gradient) - the bits of
        ``kg_step`` and of ``transE(...).backward(); torch.optim.Adam.step()``.  Any other optimiser or size loops over
        ``kg_step``.  ``.grad``: None on both parameters afterwards, on either route (see the class)."""
        from .optim import FusedAdam, _StepRoute, _fused_phase
        ent, rel = self.entity_embed.weight, self.relation_embed.weight
        lam = self.reg_lambda_kg if reg_lambda_kg is None else reg_lambda_kg
        if h.dim() != 2 or r.shape != h.shape or pos_t.shape != h.shape or neg_t.shape != h.shape:
            raise ValueError("kg_phase: h, r, pos_t, neg_t must share one (n_iterations, batch) shape")
        n_it, b = h.shape
        fused = n_it > 0 and isinstance(optimizer, FusedAdam) and self._kernels_apply(b)
        hyper = optimizer.kg_state((ent, rel)) if fused else None
        if hyper is None:
            if n_it == 0:
                ent.grad = rel.grad = None
                return torch.zeros(0, dtype=torch.float32, device=ent.device)
            # (kg_step hands back its persistent loss buffer: copy it before the next iteration overwrites it)
            return torch.stack([self.kg_step(h[i], r[i], pos_t[i], neg_t[i], optimizer, lam).clone() for i in range(n_it)])
        n, d, n_rel = ent.shape[0], ent.shape[1], rel.shape[0]
        route = _StepRoute(lambda *ids: ops.transe_presort(*ids, n, n_rel), ops.transe_adam_step, ops.TransEAdamState,
                           (n, d, n_rel, b, str(ent.device)), "_kg_phase_state")
        losses = _fused_phase(self, route, (ent, rel), _i32((h, r, pos_t, neg_t)), optimizer, hyper, lam)
        ent.grad = rel.grad = None
        return losses

    def readout(self, interaction_relation, n_users_range, item_range):
        """The N x dim table the recommendation metrics rank with: user rows ``u_user + u_rel`` (rel = the interaction
        relation), item rows ``u_item``, every other row ``u_entity``.  Item rows have unit length, so for a user query
        q, ``-|q - i|^2 = 2 q . i - |q|^2 - 1`` orders the items exactly as ``q . i`` does: ``metrics.calc_recall_ndcg``,
        ``calc_metrics``, ``calc_rank_metrics`` and ``recommend`` evaluate CFKG unchanged.  ``n_users_range`` and
        ``item_range`` are (lo, hi) row ranges."""
        ent, rel = self.entity_embed.weight, self.relation_embed.weight
        (u0, u1), (i0, i1) = n_users_range, item_range
        if not (0 <= u0 <= u1 <= ent.shape[0] and 0 <= i0 <= i1 <= ent.shape[0]) or max(u0, i0) < min(u1, i1):
            raise ValueError("readout: user rows %r and item rows %r must be disjoint ranges inside [0, %d]"
                             % ((u0, u1), (i0, i1), ent.shape[0]))
        if not 0 <= int(interaction_relation) < rel.shape[0]:
            raise IndexError("readout: relation %r outside [0, %d)" % (interaction_relation, rel.shape[0]))
        table = F.normalize(ent, p=2, dim=1)
        shift = torch.zeros_like(table)
        shift[u0:u1] = F.normalize(rel[int(interaction_relation)].unsqueeze(0), p=2, dim=1)
        return table + shift

    def load_pretrained(self, user_embed, item_embed, n_users):
        """BPR-MF embeddings into the user and item rows of the entity table (the table ``readout`` ranks with)."""
        load_pretrained_rows(self.entity_embed.weight, user_embed, item_embed, n_users)


class CKE(LinkPrediction, nn.Module):
    """Collaborative knowledge-base embedding: a TransR part - ``entity_embed``, ``relation_embed``, ``W_R``, trained by
    ``KGATPropagation``'s own ``transR`` / ``kg_step`` / ``kg_phase`` - and a CF table ``cf_embed`` (n_entities x dim);
    an item's vector is its CF row plus its entity embedding.  ``get_loss`` is the fused BPR loss
    (``KGATPropagation.get_loss``); through autograd its gradient reaches ``cf_embed`` and the items' ``entity_embed``
    rows.  As in ``KGATPropagation``, ``kg_step`` leaves every parameter's ``.grad`` None."""

    def __init__(self, n_entities, n_relations, dim=64, relation_dim=64, reg_lambda_kg=0.01, reg_lambda_cf=0.01):
        super().__init__()
        self._n_entities, self._n_relations = int(n_entities), int(n_relations)
        self.reg_lambda_kg = float(reg_lambda_kg)
        self._reg_lambda_gnn = float(reg_lambda_cf)   # (the name get_loss reads)
        self.entity_embed = nn.Embedding(n_entities, dim)
        self.relation_embed = nn.Embedding(n_relations, relation_dim)
        self.W_R = nn.Parameter(torch.empty(n_relations, dim, relation_dim))
        nn.init.xavier_uniform_(self.W_R, gain=nn.init.calculate_gain("relu"))
        self.cf_embed = nn.Embedding(n_entities, dim)
        # Xavier tables, as the KGAT release initialises its baselines: the readout ADDS the two tables, and the CF scores
        # are plain dot products - with nn.Embedding's N(0, 1) rows (norm 8 at dim 64) the BPR loss starts at 6 instead
        # of ln 2 and the entity rows, whose scale the normalised TransR loss never sees, swamp the CF rows (planted
        # run, lr 0.03, recall@20 after three epochs: 0.032 with N(0, 1), 0.448 with these)
        for table in (self.entity_embed, self.relation_embed, self.cf_embed):
            nn.init.xavier_uniform_(table.weight)

    transR = KGATPropagation.transR
    kg_step = KGATPropagation.kg_step
    kg_phase = KGATPropagation.kg_phase
    get_loss = KGATPropagation.get_loss

    def readout(self, item_range):
        """``cf_embed`` with ``entity_embed`` added on the item rows [lo, hi): differentiable."""
        lo, hi = item_range
        cf, ent = self.cf_embed.weight, self.entity_embed.weight
        if not 0 <= lo <= hi <= cf.shape[0]:
            raise ValueError("readout: item rows %r outside [0, %d]" % ((lo, hi), cf.shape[0]))
        return torch.cat([cf[:lo], cf[lo:hi] + ent[lo:hi], cf[hi:]], 0)

    def load_pretrained(self, user_embed, item_embed, n_users):
        """BPR-MF embeddings into the user and item rows of ``cf_embed`` (the table ``readout`` ranks with)."""
        load_pretrained_rows(self.cf_embed.weight, user_embed, item_embed, n_users)
