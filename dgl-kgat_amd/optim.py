"""``FusedAdam``: torch.optim.Adam (the optimiser of reference kgat.py:85) with the whole step as ONE launch of
``kgat_adam_step_f32`` over every parameter that has a gradient.

Same hyper-parameters, same state (``step`` / ``exp_avg`` / ``exp_avg_sq`` per parameter: a ``state_dict`` moves
between this class and ``torch.optim.Adam``), same dense semantics - the reference's embedding table moves in every
step, also in rows whose gradient is zero.  fp32 HIP parameters only (anything else raises: there is no fallback);
``amsgrad`` / ``weight_decay`` / ``maximize`` are not part of the reference's call and are refused.

Global-norm gradient clipping (reference kgat.py:32 ``--grad_norm``, kgat.py:162 ``clip_grad_norm_`` between backward
and step) comes in two forms: ``FusedAdam.step(max_grad_norm=c)``, which applies the clip coefficient inside the Adam
launch, and ``clip_grad_norm_``, torch's function on this package's kernels for any other optimiser."""
import ctypes as C
from collections import namedtuple

import torch

from . import _lib, ops
from ._lib import KGATLibraryError, check


def clip_grad_norm_(parameters, max_norm, norm_type=2.0):
    """``torch.nn.utils.clip_grad_norm_(parameters, max_norm)`` on the HIP kernels: the global 2-norm of the gradients
    (``ops.grad_norm``), then every gradient scaled IN PLACE by min(max_norm / (norm + 1e-6), 1) in one launch per 16
    tensors.  Returns the total norm (a 0-dim device tensor), as torch does; nothing is read back to the host, a
    non-finite norm propagates into the gradients (torch's ``error_if_nonfinite=False``).  Only ``norm_type=2``."""
    if float(norm_type) != 2.0:
        raise NotImplementedError("clip_grad_norm_: norm_type=%r (the reference clips by the 2-norm, kgat.py:162)" % (norm_type,))
    max_norm = ops.check_max_norm(max_norm)
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.tensor(0.0)
    for g in grads:
        if g.is_sparse or not g.is_cuda or g.dtype != torch.float32 or not g.is_contiguous():
            raise KGATLibraryError("clip_grad_norm_: gradients must be contiguous dense float32 HIP tensors (got %s on %s)"
                                   % (g.dtype, g.device))
    with torch.no_grad():
        norm, coef = ops.grad_norm(grads, max_norm)
        ops.scale_grads(grads, coef)
    return norm


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, zero_grads=False):
        if weight_decay != 0 or amsgrad:
            raise NotImplementedError("FusedAdam covers the reference's optim.Adam(parameters, lr): no weight decay, no amsgrad")
        if not 0.0 <= lr or not 0.0 <= eps or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("invalid Adam hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0, amsgrad=False))
        self._zero_grads = bool(zero_grads)   # also clear the gradients in the same pass (zero_grad(set_to_none=False))
        self.last_grad_norm = None            # step(max_grad_norm=c) without norm_out: that step's norm (0-dim, device)

    @torch.no_grad()
    def step(self, closure=None, *, max_grad_norm=None, norm_out=None):
        """One Adam step.  ``max_grad_norm=c`` (per call: the reference shares one Adam between its two phases and
        clips only in the CF loop) first takes ONE global 2-norm over every parameter that has a gradient - all
        parameter groups, all launches of 16 - and applies min(c / (norm + 1e-6), 1) to each gradient element inside the
        Adam launch: the bits of ``torch.nn.utils.clip_grad_norm_(params, c)`` followed by the plain step, at two extra
        launches and one extra read of the gradients, with norm and coefficient staying on the device.  The norm goes to
        ``norm_out`` (a 1-element fp32 device tensor or view) if given, else to ``self.last_grad_norm``.  The one
        difference from torch's in-place clip: the stored gradient is read, not rewritten - without ``zero_grads`` it
        keeps its unclipped bits after the step.  A non-finite norm propagates into the parameters (torch's
        ``error_if_nonfinite=False``).  ``max_grad_norm=None``: the plain step."""
        if max_grad_norm is not None:
            max_grad_norm = ops.check_max_norm(max_grad_norm)
        elif norm_out is not None:
            raise ValueError("norm_out needs max_grad_norm")
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        cap = lib.kgat_adam_max_tensors()
        coef, contiguous = None, {}
        if max_grad_norm is not None:
            with_grad = [p for group in self.param_groups for p in group["params"] if p.grad is not None]
            for p in with_grad:
                if not p.is_cuda or p.dtype != torch.float32 or p.grad.is_sparse or p.grad.dtype != torch.float32:
                    raise KGATLibraryError("FusedAdam: parameters must be contiguous float32 HIP tensors with dense "
                                           "gradients (got %s on %s)" % (p.dtype, p.device))
            if len({p.device for p in with_grad}) > 1:
                raise KGATLibraryError("FusedAdam: max_grad_norm takes one norm over all parameters; they are on %s"
                                       % ", ".join(sorted({str(p.device) for p in with_grad})))
            contiguous = {id(p): p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in with_grad}
            norm, coef = ops.grad_norm([contiguous[id(p)] for p in with_grad], max_grad_norm, norm_out=norm_out)
            if norm_out is None:
                self.last_grad_norm = norm
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.grad is not None]
            for p in ps:
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                    raise KGATLibraryError("FusedAdam: parameters must be contiguous float32 HIP tensors (got %s on %s)"
                                           % (p.dtype, p.device))
                if p.grad.is_sparse:
                    raise KGATLibraryError("FusedAdam: sparse gradients are outside the reference's dense Adam")
                st = self.state[p]
                if not st:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            # one launch per device and per `cap` tensors (a launch runs on ONE device's current stream: ADVICE round 5)
            by_dev = {}
            for p in ps:
                by_dev.setdefault(p.device, []).append(p)
            chunks = [(dv, lst[lo:lo + cap]) for dv, lst in by_dev.items() for lo in range(0, len(lst), cap)]
            for dv, chunk in chunks:
                n = len(chunk)
                steps = []
                for p in chunk:
                    st = self.state[p]
                    st["step"] += 1                      # (a CPU scalar tensor, as torch.optim.Adam keeps it)
                    steps.append(int(st["step"]))
                grads = [contiguous[id(p)] if coef is not None else
                         p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in chunk]
                arr_p = (C.c_void_p * n)(*[p.data_ptr() for p in chunk])
                arr_g = (C.c_void_p * n)(*[g.data_ptr() for g in grads])
                arr_m = (C.c_void_p * n)(*[self.state[p]["exp_avg"].data_ptr() for p in chunk])
                arr_v = (C.c_void_p * n)(*[self.state[p]["exp_avg_sq"].data_ptr() for p in chunk])
                arr_n = (C.c_int64 * n)(*[p.numel() for p in chunk])
                arr_t = (C.c_int64 * n)(*steps)
                zero = self._zero_grads and all(g is p.grad for g, p in zip(grads, chunk))
                with torch.cuda.device(dv):
                    if coef is not None:
                        check(lib.kgat_adam_step_clipped_f32(
                            n, arr_n, arr_p, arr_g, arr_m, arr_v, arr_t, float(group["lr"]), float(group["betas"][0]),
                            float(group["betas"][1]), float(group["eps"]), int(zero), coef.data_ptr(),
                            torch.cuda.current_stream(dv).cuda_stream), "kgat_adam_step_clipped_f32")
                        continue
                    check(lib.kgat_adam_step_f32(n, arr_n, arr_p, arr_g, arr_m, arr_v, arr_t, float(group["lr"]),
                                                 float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]),
                                                 int(zero), torch.cuda.current_stream(dv).cuda_stream),
                          "kgat_adam_step_f32")
        return loss

    def kg_state(self, params):
        """For KGATPropagation.kg_phase: the Adam state of `params` (created as step() creates it), and the hyper-parameters
        they share - None when they sit in groups with different hyper-parameters."""
        hyper = None
        for p in params:
            grp = next((g for g in self.param_groups if any(q is p for q in g["params"])), None)
            if grp is None:
                return None
            h = (float(grp["lr"]), float(grp["betas"][0]), float(grp["betas"][1]), float(grp["eps"]))
            if hyper is not None and h != hyper:
                return None
            hyper = h
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                return None
            st = self.state[p]
            if not st:
                st["step"] = torch.tensor(0.0)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return hyper


# What a model's phase method hands to _fused_phase: presort(*ids) -> (sorted, stride); step = the ops.*_adam_step of
# the model; state(*key[:-1], device) makes the ops.StepState, kept on the model as attribute `cache` while `key`
# (sizes, then str(device)) stays the same.
_StepRoute = namedtuple("_StepRoute", "presort step state key cache")


def _fused_phase(model, route, params, ids, optimizer, hyper, reg_lambda):
    """The loop of a fused phase (KGATPropagation.kg_phase / mf_phase, CFKG.kg_phase), once the method has decided
    that the fused route applies: `ids` are contiguous int32 (n_iterations, batch) tensors, `hyper` is what
    ``optimizer.kg_state(params)`` returned.  Every batch is sorted up front, iteration i is one ``route.step`` call on
    row i of the ids - in place on `params` and on the optimiser's exp_avg / exp_avg_sq, whose pointers are read once -
    and the step counts go back into the optimiser's state at the end.  Returns the n_iterations losses (device
    tensor).  ``.grad`` is not touched: that policy is the caller's."""
    st = getattr(model, route.cache, None)
    if st is None or st.key != route.key:
        st = route.state(*route.key[:-1], params[0].device)
        setattr(model, route.cache, st)
    n_it = ids[0].shape[0]
    losses = torch.empty(n_it, dtype=torch.float32, device=params[0].device)
    with torch.no_grad():
        sorted_all, stride = route.presort(*ids)
        states = [optimizer.state[p] for p in params]
        arr_m = (C.c_void_p * len(params))(*[s_["exp_avg"].data_ptr() for s_ in states])
        arr_v = (C.c_void_p * len(params))(*[s_["exp_avg_sq"].data_ptr() for s_ in states])
        steps = [int(s_["step"]) for s_ in states]
        data = [p.detach() for p in params]
        lr, b1, b2, eps = hyper
        for i in range(n_it):
            steps = [t + 1 for t in steps]
            route.step(*[t[i] for t in ids], sorted_all[i * stride:(i + 1) * stride], *data, arr_m, arr_v, steps, lr, b1, b2,
                       eps, reg_lambda, losses[i:i + 1], st)
        for s_, t in zip(states, steps):
            s_["step"].fill_(float(t))
    return losses
