"""Flat-buffer Adam: all parameters (and their gradients) of a model are views into ONE contiguous
fp32 buffer, so the optimiser step is one esc_adam_step launch and the data-parallel gradient
exchange is one RCCL all-reduce of `flat_grad`.  Arithmetic = torch.optim.Adam
(reference run_graphcount.py:478: Adam(model.parameters(), lr), defaults betas=(0.9,0.999), eps=1e-8).
"""
import math

import torch

from . import _native as nv
from .parallel import FlatBucket


def _several_ranks():
    import torch.distributed as dist
    return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1


class FlatAdam(FlatBucket):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, late=None, weight_decay=0.0):
        """weight_decay: decoupled (torch.optim.AdamW: p *= 1 - lr * weight_decay before the update), as one scaling of the flat
        parameter buffer; 0.0 adds no launch and changes no bit."""
        params = [p for p in params]
        if params and params[0].device.type != "cuda":
            raise RuntimeError("FlatAdam runs on the HIP device only; there is no CPU fallback")
        super().__init__(params, late=late)
        self.exp_avg = torch.zeros_like(self.flat_param)
        self.exp_avg_sq = torch.zeros_like(self.flat_param)
        self.param_groups = [dict(lr=lr, betas=betas, eps=eps, params=self.params)]
        if weight_decay:                                  # (the key exists only then: checkpoints without decay keep their layout)
            self.param_groups[0]["weight_decay"] = weight_decay
        self.step_count = 0
        self._seam_versions = None        # write_versions() as StepEngine.end_step() saw them

    def write_versions(self):
        """torch's in-place version counters of everything step() reads or writes: the gradient store (every p.grad is a view
        of it), the flat parameter buffer and every parameter (a re-homed parameter keeps a counter of its own), the two moment
        buffers.  A torch op that writes one of them moves a counter; the library's own launches, which go by raw address, and
        writes through `.data` do not."""
        return (self._grad_store._version, self.flat_param._version, self.exp_avg._version, self.exp_avg_sq._version,
                tuple(p._version for p in self.params))

    def step(self, grad_denom=None):
        """One Adam update.  grad_denom: device scalar the gradients are divided by inside the launch (the global
        target count returned by `all_reduce_sum`)."""
        g = self.param_groups[0]
        self.step_count += 1
        if g.get("weight_decay"):
            self.flat_param.mul_(1.0 - float(g["lr"]) * float(g["weight_decay"]))
        elif (grad_denom is None and self.early_numel < self.numel and self._seam_versions is not None and
              self._seam_versions == self.write_versions() and not _several_ranks()):
            # the plain step of a bucket with a `late` part: behind a two-stream StepEngine step over these very buffers the library
            # updates that part on the engine's edge stream (escgnn_step.h); it finds out by the addresses, and anywhere else this
            # is the call below.  That launch is NOT ordered behind what the caller queued on its stream since end_step(): only
            # when no torch op has written a gradient, a parameter or the optimiser state since then (clipping, scaling,
            # accumulation, a weight clamp: all of them show in the version counters end_step() noted).
            nv.call("esc_engine_adam_step", nv.ptr(self.flat_param), nv.ptr(self.flat_grad), nv.ptr(self.exp_avg),
                    nv.ptr(self.exp_avg_sq), self.flat_param.numel(), self.early_numel, float(g["lr"]), float(g["betas"][0]),
                    float(g["betas"][1]), float(g["eps"]), self.step_count, nv.stream())
            return
        nv.call("esc_adam_step_scaled", nv.ptr(self.flat_param), nv.ptr(self.flat_grad), nv.ptr(self.exp_avg),
                nv.ptr(self.exp_avg_sq), self.flat_param.numel(), float(g["lr"]), float(g["betas"][0]),
                float(g["betas"][1]), float(g["eps"]), self.step_count, nv.ptr(grad_denom), nv.stream())

    def clip_scale(self, max_norm):
        """device scalar max((|g|_2 + 1e-6) / max_norm, 1) over the flat gradient buffer: dividing the gradients by it is
        torch.nn.utils.clip_grad_norm_(params, max_norm).  Hand it to step(grad_denom=...): the division rides on the Adam
        launch, and nothing is read back."""
        norm = torch.linalg.vector_norm(self.flat_grad)
        return ((norm + 1e-6) / float(max_norm)).clamp_(min=1.0).reshape(1)

    def state_dict(self):
        return dict(step=self.step_count, exp_avg=self.exp_avg, exp_avg_sq=self.exp_avg_sq,
                    param_groups=[{k: v for k, v in g.items() if k != "params"} for g in self.param_groups])

    def load_state_dict(self, sd):
        self.step_count = int(sd["step"])
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        for g, s in zip(self.param_groups, sd["param_groups"]):
            g.update(s)


class ReduceLROnPlateau(object):
    """torch.optim.lr_scheduler.ReduceLROnPlateau(mode='min', threshold=1e-4 rel) as configured at
    reference run_graphcount.py:479-480 (factor=lr_decay_factor, patience, min_lr=1e-5); works on any
    object with `param_groups`."""

    def __init__(self, optimizer, mode="min", factor=0.1, patience=10, min_lr=0.0, threshold=1e-4):
        assert mode == "min"
        self.optimizer, self.factor, self.patience, self.min_lr, self.threshold = optimizer, factor, patience, min_lr, threshold
        self.best, self.num_bad = float("inf"), 0

    def step(self, metric):
        m = float(metric)
        if m < self.best * (1.0 - self.threshold):
            self.best, self.num_bad = m, 0
        else:
            self.num_bad += 1
        if self.num_bad > self.patience:
            for g in self.optimizer.param_groups:
                new = max(g["lr"] * self.factor, self.min_lr)
                if g["lr"] - new > 1e-8:
                    g["lr"] = new
            self.num_bad = 0


class CosineWithWarmup(object):
    """The `cosine_with_warmup` schedule of the reference's graph transformer (GraphGPS/graphgps/optimizer/extra_optimizers.py,
    get_cosine_schedule_with_warmup with num_cycles = 0.5, stepped once per epoch through torch's LambdaLR): lr = base_lr *
    factor(epoch), factor linear from 1e-6 up to 1 over the warm-up epochs, then half a cosine down to 0 at max_epoch.  Works on
    any object with `param_groups`, like ReduceLROnPlateau above; step() takes and ignores a metric so that
    harness.fit_regression can drive it."""

    def __init__(self, optimizer, num_warmup_epochs, max_epoch):
        self.optimizer, self.num_warmup_epochs, self.max_epoch = optimizer, int(num_warmup_epochs), int(max_epoch)
        self.base_lrs = [g["lr"] for g in optimizer.param_groups]
        self.last_epoch = -1
        self.step()                                        # LambdaLR applies factor(0) on construction

    def factor(self, epoch):
        if epoch < self.num_warmup_epochs:
            return max(1e-6, float(epoch) / float(max(1, self.num_warmup_epochs)))
        progress = float(epoch - self.num_warmup_epochs) / float(max(1, self.max_epoch - self.num_warmup_epochs))
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * 0.5 * 2.0 * progress)))

    def step(self, metric=None):
        self.last_epoch += 1
        for g, base in zip(self.optimizer.param_groups, self.base_lrs):
            g["lr"] = base * self.factor(self.last_epoch)
