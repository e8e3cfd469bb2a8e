"""DeiT distillation -- MI355X-native counterpart of the reference ``src/myrtle_vision/models/distill.py``.

Same classes (``DistillableViT``, ``DistillWrapper``), constructor arguments, parameter names (``distillation_token``,
``distill_mlp.0.*``, ``distill_mlp.1.*``, ``student.*``, ``teacher.*``) and loss (distill.py:142-151) as the reference.  The
reference's ``DistillableViT.forward`` is stale -- it reads ``self.pool``, ``self.to_latent`` and ``self.mlp_head``, which its ``ViT``
no longer has -- so what runs here is what that code evidently intends (DeiT, Touvron et al. 2021) on the ``ViT`` of
this package: a learned distillation token appended behind the positional add, a LayerNorm + Linear head on its output row, and the
head trained against a frozen teacher's logits.

Nothing here adds a matrix kernel: the token is appended by ``F.token_append`` (``mv_det_append_*`` with one row), the head is
``F.cls_head(..., row=T-1)`` and the loss with both gradients and the student's arg-max is one launch of ``mv_distill_loss``.

Extensions, each off by default: ``DistillWrapper(distillation_type="hard")`` (DeiT's hard-label variant) and the ``lam`` /
``smoothing`` / ``pair_flip`` / ``return_argmax`` keywords of ``DistillWrapper.forward`` (the Mixup recipe, and the arg-max that
spares the training loop the reference's second student pass, classification/train.py:247-253).
"""
from typing import Optional

import torch
from torch import nn

from myrtle_vision.hip import functional as F
from myrtle_vision.hip import ops
from myrtle_vision.models.vit import ClassificationDecoder, LayerNorm, Linear, ViT, _plain


class DistillableViT(ViT):
    """A ``ViT`` whose ``forward`` takes an optional distillation token.  It adds no parameter, buffer or module: state-dict keys and
    their order are those of a ``ViT`` with the same arguments.  Classification only."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if not isinstance(self.decoder, ClassificationDecoder):
            raise ValueError(f"DistillableViT is classification-only: decoder={kwargs.get('decoder')!r} has no class token to distil")
        self.args = args
        self.kwargs = kwargs
        self.dim = kwargs["dim"]
        self.num_classes = kwargs["num_classes"]

    def to_vit(self):
        """A plain ``ViT`` with the same arguments and weights (reference distill.py:23-27)."""
        v = ViT(*self.args, **self.kwargs)
        v.load_state_dict(self.state_dict())
        return v

    def distill_sequence(self, img: torch.Tensor, distill_token: torch.Tensor):
        """-> (class logits fp32 [B, C], the whole output sequence fp32 [B, T0 + 1, D]); the distillation token's output is its last
        row.  ``prune_dead_tokens`` is treated as off: with a second live row the last block's patch rows are still dead, but the
        slice to the cls row would drop the distillation row with them."""
        if not self._embed_fusable():
            raise ValueError("a distillation token needs q_format 'FP32': the fake-quantised embedding path has no stub for it")
        tail, self.transformer.cls_only_tail = self.transformer.cls_only_tail, False
        try:
            with ops.segments(ops.prec_segments(self.precision)):
                x = self._backbone(img, extra_token=distill_token)
                with self.cm_mlp_head:
                    # the decoder reads row 0 of every image, T * D apart: the sequence without its last row needs no copy
                    logits = self.dequant_output(self.decoder(x))
        finally:
            self.transformer.cls_only_tail = tail
        return logits, x

    def forward(self, img: torch.Tensor, distill_token: Optional[torch.Tensor] = None):
        """Without a token exactly ``ViT.forward``; with one -> (class logits [B, C], distillation-token output [B, D]), both fp32
        (reference distill.py:73-85)."""
        if distill_token is None:
            return super().forward(img)
        logits, x = self.distill_sequence(img, distill_token)
        return logits, x[:, -1]


class DistillWrapper(nn.Module):
    """Knowledge-distillation wrapper (reference distill.py:90-151): ``forward(img, labels)`` -> the scalar
    ``alpha * CE(student(img), labels) + (1 - alpha) * T^2 * KL(softmax(teacher(img) / T) || softmax(distill_head / T))``.

    The teacher is frozen: its parameters get ``requires_grad_(False)`` (so ``ParamArena`` and the gradient exchange never see them), it
    runs under ``torch.no_grad()`` and it stays in eval mode through ``train()``.  The student runs once per step."""

    def __init__(self, *, teacher: nn.Module, student: DistillableViT, temperature: float = 1.0, alpha: float = 0.5,
                 distillation_type: str = "soft"):
        super().__init__()
        assert isinstance(student, DistillableViT), "student must be a vision transformer"
        if distillation_type not in ops.DISTILL_MODES:
            raise ValueError(f"distillation_type must be 'soft' or 'hard', got {distillation_type!r}")
        self.teacher = teacher
        self.student = student
        dim, num_classes = student.dim, student.num_classes
        self.temperature = temperature
        self.alpha = alpha
        self.distillation_type = distillation_type

        self.distillation_token = nn.Parameter(torch.randn(1, 1, dim))
        self.distill_mlp = nn.Sequential(
            LayerNorm(dim),
            Linear(dim, num_classes),
        )
        for m in self.distill_mlp:
            m.precision = student.precision
        self.teacher.requires_grad_(False)
        self.teacher.eval()

    def train(self, mode: bool = True):
        super().train(mode)
        self.teacher.eval()                              # a frozen teacher has no training mode (dropout, drop path)
        return self

    def unused_parameter_names(self):
        """The student's never-used detection parameters under their names here (``create_optimizer`` leaves them out)."""
        return tuple("student." + n for n in self.student.unused_parameter_names())

    def head_state_dict(self):
        """``distillation_token`` and ``distill_mlp.*`` on the host: the checkpoint's ``"distiller"`` entry."""
        return {k: v.detach().cpu().clone() for k, v in self.state_dict().items()
                if k == "distillation_token" or k.startswith("distill_mlp.")}

    def load_head_state_dict(self, state):
        expected = set(self.head_state_dict())
        if set(state) != expected:
            raise KeyError(f"distiller state has keys {sorted(state)}, expected {sorted(expected)}")
        own = self.state_dict()
        with torch.no_grad():
            for k, v in state.items():
                own[k].copy_(v)

    def _distill_logits(self, x):
        norm, linear = self.distill_mlp
        if _plain(norm, LayerNorm) and _plain(linear, Linear):
            return F.cls_head(x, norm.weight, norm.bias, linear.weight, linear.bias, norm.precision, row=x.shape[1] - 1)
        return F.cast(self.distill_mlp(x[:, -1]), torch.float32)

    def forward(self, img: torch.Tensor, labels: torch.Tensor, temperature: Optional[float] = None, alpha: Optional[float] = None,
                lam: float = 1.0, smoothing: float = 0.0, pair_flip: bool = False, return_argmax: bool = False):
        """``lam``, ``smoothing``, ``pair_flip`` (extensions; the reference's plain cross entropy is lam=1, smoothing=0,
        pair_flip=False): the student's cross entropy against the Mixup / label-smoothing target of ``F.soft_cross_entropy``.
        ``return_argmax`` (extension, reference: False): -> (loss, arg-max of the student's class logits, int64 [B])."""
        alpha = alpha if alpha is not None else self.alpha
        T = temperature if temperature is not None else self.temperature

        with torch.no_grad():
            teacher_logits = self.teacher(img)
        if teacher_logits.dim() != 2:
            raise ValueError(f"the teacher must return [B, C] class logits, got {tuple(teacher_logits.shape)}")

        student_logits, x = self.student.distill_sequence(img, self.distillation_token)
        distill_logits = self._distill_logits(x)
        with ops.segments(ops.prec_segments(self.student.precision)):
            return F.distill_loss(student_logits, distill_logits, teacher_logits.float(), labels, T, alpha, self.distillation_type,
                                  lam, smoothing, pair_flip, return_argmax=return_argmax)
