"""Drop-in for the reference's ``models.py`` on MI355X.

Same public surface (reference ``models.py:7-81``): ``ChannelAttention(in_channels,
reduction_ratio=4)`` and ``CnnGruAttentionModel(in_channels, num_classes,
cnn_out_channels=32, gru_hidden_size=64, gru_num_layers=2, dropout=0.5)`` are
``nn.Module``s with the reference's ``state_dict`` keys, shapes and default
initialisers (drawn in the same order, so the same ``torch.manual_seed`` gives the
same initial weights).  The sub-modules are parameter CONTAINERS only: all arithmetic
runs in libmsig_hip.so on the flat parameter buffer the parameters are views of.
There is no CPU fallback — a CPU input raises.

``CnnGruModel`` is the ``cnn_gru`` baseline the reference's README compares against but
never defines: ``CnnGruAttentionModel`` without ``channel_attention`` (include/msig_cg.h,
DESIGN.md section 13).
"""
from __future__ import annotations

import itertools
import math

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib as L
from .runtime import EmbeddedEngine, Engine

_instance_counter = itertools.count()


class ChannelAttention(nn.Module):
    """Container for the squeeze-excite gate's two bias-free Linear layers (models.py:12-22)."""

    def __init__(self, in_channels, reduction_ratio=4):
        super().__init__()
        hidden = in_channels // reduction_ratio
        self.avg_pool = nn.AdaptiveAvgPool1d(1)
        self.fc = nn.Sequential(nn.Linear(in_channels, hidden, bias=False), nn.ReLU(inplace=True),
                                nn.Linear(hidden, in_channels, bias=False), nn.Sigmoid())

    def forward(self, x):
        """models.py:24-31 on its own: x * sigmoid(fc(mean_T(x)))[:, :, None] through msig_channel_attention (gate_kernel + one
        scaling pass).  Inside CnnGruAttentionModel the product is never written (the gate is folded into conv1's taps); this
        stand-alone forward is inference-only — gradients flow through the model's fused path, not through this call."""
        import ctypes as C
        if not x.is_cuda:
            raise RuntimeError("ChannelAttention.forward needs a GPU tensor: the MI355X path has no CPU fallback")
        if x.dtype != torch.float32 or x.dim() != 3 or x.shape[1] != self.fc[0].in_features:
            raise ValueError(f"expected float32 (B,{self.fc[0].in_features},T) input, got {x.dtype} {tuple(x.shape)}")
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise RuntimeError("the stand-alone ChannelAttention.forward is inference-only: call it under torch.no_grad(), "
                               "or train through CnnGruAttentionModel")
        x = x.contiguous()
        B, Cc, T = x.shape
        w1, w2 = self.fc[0].weight, self.fc[2].weight
        if w1.device != x.device:
            raise RuntimeError(f"ChannelAttention weights are on {w1.device}, input on {x.device}")
        out = torch.empty_like(x)
        s = torch.empty((B, Cc), dtype=torch.float32, device=x.device)
        scratch = torch.empty(B * (Cc + Cc // 4) + 4, dtype=torch.float32, device=x.device)
        st = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
        L.check(L.lib().msig_channel_attention(x.data_ptr(), w1.contiguous().data_ptr() if w1.numel() else None,
                                               w2.contiguous().data_ptr() if w2.numel() else None, B, Cc, T, out.data_ptr(),
                                               s.data_ptr(), scratch.data_ptr(), st), "msig_channel_attention")
        return out


class _GruParams(nn.Module):
    """nn.GRU's parameters (names, shapes, U(-1/sqrt(H), 1/sqrt(H)) init in nn.GRU's order)
    without nn.GRU itself, so no MIOpen weight flattening ever touches them."""

    def __init__(self, input_size, hidden_size, num_layers):
        super().__init__()
        self.input_size, self.hidden_size, self.num_layers, self.bidirectional = input_size, hidden_size, num_layers, True
        for layer in range(num_layers):
            isz = input_size if layer == 0 else 2 * hidden_size
            for sfx in ("", "_reverse"):
                self.register_parameter(f"weight_ih_l{layer}{sfx}", nn.Parameter(torch.empty(3 * hidden_size, isz)))
                self.register_parameter(f"weight_hh_l{layer}{sfx}", nn.Parameter(torch.empty(3 * hidden_size, hidden_size)))
                self.register_parameter(f"bias_ih_l{layer}{sfx}", nn.Parameter(torch.empty(3 * hidden_size)))
                self.register_parameter(f"bias_hh_l{layer}{sfx}", nn.Parameter(torch.empty(3 * hidden_size)))
        stdv = 1.0 / math.sqrt(hidden_size)
        for w in self.parameters():
            nn.init.uniform_(w, -stdv, stdv)

    def forward(self, *a, **k):
        raise RuntimeError("the GRU runs inside libmsig_hip.so; call CnnGruAttentionModel")


class _MsigFunction(torch.autograd.Function):
    """model(inputs) with autograd: forward = msig_forward, backward = msig_backward (input gradient through msig_batch.dx).  An
    eval-mode forward keeps what the backward reads (msig_batch.keep_for_backward) only when autograd may ask for it: grad mode on
    and the input or a parameter requiring grad.  Its logits are the same bits either way."""

    @staticmethod
    def forward(ctx, model, keep, x, *params):
        eng = model._engine
        training = model.training
        step = model._bump_step() if training else 0
        keep = bool(keep) and not training
        b = eng.forward(x, None, training=training, dropout_p=model.dropout_p, seed=model._seed, step=step, keep_for_backward=keep)
        ctx.model, ctx.batch, ctx.token, ctx.training, ctx.kept = model, b, model._bump_token(), training, training or keep
        return eng.region("LOGITS", torch.float32, (x.shape[0], model.num_classes)).clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, dlogits):
        model = ctx.model
        if not ctx.kept:
            raise RuntimeError("backward through a model.eval() forward that kept nothing for it: it ran with autograd disabled or "
                               "with neither the input nor any parameter requiring grad")
        if ctx.token != model._token:
            raise RuntimeError("the activations of this forward were overwritten by a later forward of the same model")
        eng = model._engine
        dx = None
        if ctx.needs_input_grad[2]:
            B, T = ctx.batch.shape.B, ctx.batch.shape.T
            dx = torch.empty((B, model.in_channels, T), dtype=torch.float32, device=dlogits.device)
        eng.backward(ctx.batch, dlogits, dx=dx)
        if model.embedded:
            grads = [g.clone() for g in eng.gather_grads().values()]
        else:
            grads = [g.clone() for g in eng.named_param_views(eng.grads).values()]       # the kind's tensors, in _named()'s order
        return (None, None, dx, *grads)


class _MsigModel(nn.Module):
    """What CnnGruAttentionModel and CnnGruModel share: the containers, the binding to an Engine of the model's kind, autograd."""
    kind = None

    def __init__(self, in_channels, num_classes, cnn_out_channels=32, gru_hidden_size=64, gru_num_layers=2, dropout=0.5):
        if self.kind not in L.MODEL_KINDS:
            raise TypeError(f"{type(self).__name__} has no model kind: instantiate CnnGruAttentionModel or CnnGruModel")
        super().__init__()
        if (cnn_out_channels, gru_hidden_size, gru_num_layers) not in ((32, 64, 2), (32, 32, 1)):
            raise NotImplementedError(
                "the HIP path covers the reference's two configurations: cnn_out_channels=32 with gru_hidden_size=64, "
                "gru_num_layers=2 (main.py:48-55) or gru_hidden_size=32, gru_num_layers=1 (the hierarchical experiment's second "
                f"model, main.py:35-40); got {(cnn_out_channels, gru_hidden_size, gru_num_layers)}")
        # the 32-unit one-layer model runs embedded in the 64-unit kernels (runtime.EmbeddedEngine): same state_dict as the reference's
        self.embedded = (gru_hidden_size, gru_num_layers) == (32, 1)
        self.gru_hidden_size, self.gru_num_layers = gru_hidden_size, gru_num_layers
        if not (1 <= in_channels <= L.MAX_C and 2 <= num_classes <= L.MAX_K):
            raise ValueError(f"in_channels must be 1..{L.MAX_C} and num_classes 2..{L.MAX_K}")
        self.in_channels, self.num_classes, self.dropout_p = in_channels, num_classes, float(dropout)
        # containers, created in the reference's order (models.py:43-71) so that the RNG stream matches; the baseline has no gate
        if self.kind == "cnn_gru_attention":
            self.channel_attention = ChannelAttention(in_channels)
        self.cnn_encoder = nn.Sequential(
            nn.Conv1d(in_channels, 16, kernel_size=7, stride=2, padding=3, bias=False), nn.BatchNorm1d(16), nn.ReLU(),
            nn.MaxPool1d(kernel_size=3, stride=2, padding=1),
            nn.Conv1d(16, cnn_out_channels, kernel_size=5, stride=2, padding=2, bias=False), nn.BatchNorm1d(cnn_out_channels),
            nn.ReLU(), nn.MaxPool1d(kernel_size=3, stride=2, padding=1))
        self.gru = _GruParams(cnn_out_channels, gru_hidden_size, gru_num_layers)
        self.classifier = nn.Sequential(nn.Linear(2 * gru_hidden_size, 64), nn.ReLU(), nn.Dropout(dropout), nn.Linear(64, num_classes))
        self._engine = None
        self._seed = (torch.initial_seed() * 0x9E3779B97F4A7C15 + next(_instance_counter)) % (1 << 64)
        self._step = 0
        self._token = 0

    # ---- binding of nn.Parameters / buffers to the engine's flat buffers ----------------------
    def _named(self):
        sd_params = dict(self.named_parameters())
        return [sd_params[k] for k in L.PARAM_KEYS if k in sd_params]        # the one-layer model has no *_l1* tensors

    def _grad_views(self):
        """Where the optimiser puts p.grad (same order as _named()) for the un-fused path (MsigAdam.step)."""
        eng = self._engine
        if self.embedded:
            return list(eng.small_views(eng.small_grads).values())
        return list(eng.named_param_views(eng.grads).values())

    def engine(self) -> Engine:
        """Returns the Engine whose flat buffers the parameters are views of (re-binding after
        .to(), load_state_dict(assign=True) or anything else that replaced a parameter's storage)."""
        sd_params = dict(self.named_parameters())
        dev = self.classifier[0].weight.device
        if dev.type != "cuda":
            raise RuntimeError(f"model is on {dev}: move it to the GPU (model.to('cuda')); there is no CPU fallback")
        if self._engine is None or self._engine.device != dev:
            self._engine = (EmbeddedEngine(self.in_channels, self.num_classes, dev, self.gru_hidden_size, kind=self.kind) if self.embedded
                            else Engine(self.in_channels, self.num_classes, dev, kind=self.kind))
        eng = self._engine
        views = eng.small_views() if self.embedded else eng.named_param_views()
        for k, view in views.items():                      # by key: the baseline's positions differ from the attention model's
            p = sd_params[k]
            if p.numel() and (p.data_ptr() != view.data_ptr() or p.device != dev):
                view.copy_(p.data)
                p.data = view
        bv = eng.bn_views()
        for idx in (1, 5):
            bn = self.cnn_encoder[idx]
            for name in ("running_mean", "running_var", "num_batches_tracked"):
                cur, view = bn._buffers[name], bv[f"cnn_encoder.{idx}.{name}"]
                if cur.data_ptr() != view.data_ptr() or cur.device != dev:
                    view.copy_(cur)
                    bn._buffers[name] = view
        return eng

    def set_dropout_seed(self, seed: int):
        """Dropout masks are a pure function of (seed, step, element): fix the seed for reproducible runs
        (by default it derives from torch.initial_seed() and the order of construction)."""
        self._seed = int(seed) % (1 << 64)
        self._step = 0

    def _bump_step(self):
        self._step += 1
        return self._step

    def _bump_token(self):
        self._token += 1
        return self._token

    @torch.no_grad()
    def embed(self, x):
        """Window embeddings: the (B, 2 * gru_hidden_size) vector the classifier sees, ``outputs[:, -1, :]`` (models.py:79), of an
        EVAL-mode forward whatever ``self.training`` is — running-statistics BatchNorm, no dropout.  No autograd graph; parameters,
        BatchNorm buffers, the dropout step counter and ``self.training`` are untouched (msig_ft_features: front end and GRU, no
        head launch).  What few-shot calibration caches (calibrate.HeadCalibrator) and what PCA / t-SNE plots take."""
        if not x.is_cuda:
            raise RuntimeError(f"{type(self).__name__}.embed needs a GPU tensor: the MI355X path has no CPU fallback")
        return self.engine().features(x)

    @torch.no_grad()
    def adapt_bn(self, x, alpha=1.0, inplace=False):
        """Label-free BatchNorm adaptation (AdaBN, adapt.BnAdapter, include/msig_ab.h): the four ``cnn_encoder.{1,5}.running_{mean,var}``
        tensors this model would have with the statistics of the unlabelled windows ``x`` (N, C, T) — stage 1 over the whole set,
        then stage 2 under the adapted stage 1 in its eval form — blended as ``(1 - alpha) * current + alpha * new``.  Every weight,
        ``num_batches_tracked`` and ``self.training`` are untouched; with ``inplace=False`` so are the running statistics, and
        ``inplace=True`` loads the returned tensors into the model."""
        if not x.is_cuda:
            raise RuntimeError(f"{type(self).__name__}.adapt_bn needs a GPU tensor: the MI355X path has no CPU fallback")
        from .adapt import BnAdapter
        bufs = BnAdapter([dict(model=self, x=x)], alpha=alpha).adapted_buffers(0)
        if inplace:
            self.engine().load_named(bufs)
        return bufs

    @torch.no_grad()
    def adapt_entropy(self, x, lr=1e-3, epochs=1, diversity=0.0, params="bn", batch=64, seed=0, order="shuffled", inplace=False):
        """Label-free entropy-minimisation adaptation (TENT, tta.EntropyAdapter, include/msig_tt.h): the tensors ``params`` names
        ("bn": the BatchNorm scale and shift; "bn+gate"; "all") after ``epochs`` passes of Adam at ``lr`` down the entropy of this
        model's own eval-mode predictions on the unlabelled windows ``x`` (N, C, T), less ``diversity`` times the entropy of a
        batch's mean prediction.  Returned under the reference's ``state_dict`` names.  The BatchNorm buffers,
        ``num_batches_tracked``, ``self.training``, every ``.grad`` and the dropout step counter are untouched; with
        ``inplace=False`` so is every parameter, and ``inplace=True`` loads the returned tensors into the model."""
        if not x.is_cuda:
            raise RuntimeError(f"{type(self).__name__}.adapt_entropy needs a GPU tensor: the MI355X path has no CPU fallback")
        from .tta import EntropyAdapter
        out = EntropyAdapter([dict(model=self, x=x)], lr=lr, epochs=epochs, diversity=diversity, batch=batch, params=params, seed=seed,
                             order=order).adapted_tensors(0)
        if inplace:
            named = dict(self.named_parameters())
            for k, v in out.items():
                named[k].data.copy_(v)                  # the parameters are views of the engine's buffers: this is the load
        return out

    def attribute(self, x, target="predicted", steps=32, baseline=None, bin=None, return_map=True):
        """Integrated-gradients attribution (attribute.Attributor, include/msig_at.h) of the windows ``x`` (N, C, T) in EVAL mode
        whatever ``self.training`` is: ``(x - baseline) * mean_p df/dx`` at ``steps`` midpoints of the straight path from the
        baseline (None: zero; (C,), (C, T) or (N, C, T)) to x, with f = the target's combination of the logits (a class index,
        "predicted" or a (K,) / (N, K) vector).  Returns an ``attribute.Attribution``: the map, its sums per time bin of ``bin``
        samples (None: T // 60), per channel and per window, f(x), f(baseline) and the completeness gap.  Parameters, BatchNorm
        buffers, every ``.grad``, the dropout step counter and ``self.training`` are untouched."""
        from .attribute import Attributor
        return Attributor(self, steps=steps, baseline=baseline, bin=bin).attribute(x, target, return_map)

    def channel_occlusion(self, x, target="predicted", baseline=None):
        """(N, C): f(x) - f(x with channel c set to its baseline), eval-mode forwards only (attribute.Attributor.channel_occlusion)."""
        from .attribute import Attributor
        return Attributor(self, baseline=baseline).channel_occlusion(x, target)

    def predict_mc(self, x, samples=32, seed=0, chunk=None, return_samples=False):
        """Monte-Carlo dropout (uncertainty.McDropout, include/msig_mc.h) of the windows ``x`` (N, C, T): ``samples`` stochastic
        passes with both dropout masks on at ``dropout`` and BatchNorm in its EVAL form, whatever ``self.training`` is.  Returns an
        ``uncertainty.McPrediction``: mean and std of the softmax vectors, the prediction, predictive entropy, expected entropy,
        mutual information and the vote split (with ``return_samples`` also the (N, S, K) logits).  The deterministic trunk — front
        end and GRU layer 0 — runs once per window.  Windows are cut into chunks of ``chunk`` (None: the most with chunk * samples
        <= 2048 rows); chunk j draws its masks under msig_dropout_key(seed, j, 1 / 2), so a result is a function of (weights, x,
        seed, samples, chunk) alone.  Parameters, BatchNorm buffers, ``num_batches_tracked``, ``self.training``, the dropout step
        counter and torch's RNG are untouched."""
        from .uncertainty import McDropout
        return McDropout(self, samples=samples, seed=seed, chunk=chunk).predict(x, return_samples)

    def forward(self, x):
        if isinstance(x, (list, tuple)):
            raise TypeError("this model takes one (B, C, T) tensor (trainer.py:135-140's list branch is for a dataset "
                            "the reference no longer ships)")
        if not x.is_cuda:
            raise RuntimeError(f"{type(self).__name__}.forward needs a GPU tensor: the MI355X path has no CPU fallback")
        self.engine()
        params = self._named()
        # an eval-mode forward keeps what a backward reads only when autograd may ask for one (decided here: inside
        # Function.forward grad mode is always off)
        keep = (not self.training and torch.is_grad_enabled()
                and (x.requires_grad or any(p.requires_grad for p in params)))
        return _MsigFunction.apply(self, keep, x, *params)


class CnnGruAttentionModel(_MsigModel):
    """The reference's model (models.py:34-81): ChannelAttention -> cnn_encoder -> 2-layer bidirectional GRU -> classifier."""
    kind = "cnn_gru_attention"


class CnnGruModel(_MsigModel):
    """The ``cnn_gru`` baseline of the reference's README (README.md:13,81: MODEL_TO_USE = 'cnn_gru'), which its models.py never
    defines.  Our reading: CnnGruAttentionModel with ``channel_attention`` removed —

        cnn_encoder -> permute -> GRU -> outputs[:, -1, :] -> classifier

    with the same layers, configurations ((32, 64, 2) and the embedded (32, 32, 1); others raise NotImplementedError), reference
    quirks and initialisers, drawn in the attention model's order minus the gate's two Linear layers.  Its state_dict is the
    attention model's minus ``channel_attention.fc.0.weight`` and ``channel_attention.fc.2.weight``.  Any C in 1..16.  It runs on
    include/msig_cg.h: conv1 on the raw taps, no gate launch, no gate backward."""
    kind = "cnn_gru"
