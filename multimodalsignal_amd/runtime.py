"""Device-side state of one model instance and thin wrappers over the C ABI.

`Engine` owns (through torch tensors) the flat parameter / gradient / Adam
buffers, the BatchNorm buffers and a cache of workspaces, builds the
`msig_batch` descriptor for every call and launches on torch's current HIP
stream.  It holds no arithmetic of its own.

The host never chooses among entry points: every train step is msig_sc_train_step[_multi], every forward msig_st_forward[_multi],
the widest of each form, with NULL for every optional term that is off.  The headers make that bit-safe — a NULL
msig_da, msig_kd, msig_sam, msig_dro or msig_sc, smoothing 0 with every lam 1, a NULL clip, a NULL class_weight each give the
narrower call with its launches, `kind` selects the model — and tests/test_step_dispatch_gpu.py pins it, term by term, against the
narrower entry points called directly.  A new term widens the widest call; it adds no branch here.
"""
from __future__ import annotations

import ctypes as C
import weakref
from typing import Dict, Optional, Tuple

import torch

from . import _lib as L


def _ref(desc):
    """byref of a descriptor, or None (a NULL pointer) for a term that is off."""
    return None if desc is None else C.byref(desc)


def _require_gpu(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise RuntimeError(
            f"{what} is on {t.device}: the multimodalsignal_amd path runs only on an AMD GPU through "
            "libmsig_hip.so (there is no CPU fallback; the CPU restatement lives in oracle/ and is test-only).")


class Engine:
    def __init__(self, in_channels: int, num_classes: int, device: torch.device, storage: Optional[dict] = None,
                 kind: str = "cnn_gru_attention"):
        """`storage` (FoldArena.engine): pre-allocated flat tensors "params", "grads", "exp_avg", "exp_avg_sq", "bn_state",
        "bn_count" and a "ws" byte region to use instead of allocating — the buffers of one arena of a fold batch (plus "gc", the
        arena's clip state, when the arena was built for gradient clipping, and "avg_params", "avg_bn_state", "avg_bn_count", the
        arena's weight-averaging shadow, when it was built for averaging).  `kind`:
        "cnn_gru_attention" (include/msig.h, msig_cw.h) or "cnn_gru", the baseline without ChannelAttention (include/msig_cg.h:
        its layout and its calls)."""
        if not (1 <= in_channels <= L.MAX_C) or not (2 <= num_classes <= L.MAX_K):
            raise ValueError(f"unsupported in_channels={in_channels} / num_classes={num_classes}")
        self.kind = L.check_kind(kind)
        self.C, self.K = in_channels, num_classes
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("Engine needs a cuda (HIP) device")
        L.lib()
        self.layout = L.param_layout(self.C, self.K, kind)
        self.shapes = L.param_shapes(self.C, self.K, kind)
        self.keys = L.param_keys(kind)          # (msig_param index, state_dict key) of the tensors this kind has
        self.n_flat = self.layout[-1]
        self._ws_region = None
        if storage is None:
            self.params = torch.zeros(self.n_flat, dtype=torch.float32, device=self.device)
            self.grads = torch.zeros(self.n_flat, dtype=torch.float32, device=self.device)
            self.bn_state = torch.zeros(L.BN_STATE_FLOATS, dtype=torch.float32, device=self.device)
            self.bn_count = torch.zeros(2, dtype=torch.int64, device=self.device)
            self.exp_avg: Optional[torch.Tensor] = None
            self.exp_avg_sq: Optional[torch.Tensor] = None
            self.loss_acc = torch.zeros(2, dtype=torch.float64, device=self.device)      # msig_batch.loss_acc: [sum of CE, #correct] of a pass
            self.gc_state: Optional[torch.Tensor] = None      # include/msig_gc.h clip state (float64), made by the first clipped step
            self.sam_state: Optional[torch.Tensor] = None     # include/msig_sam.h state (float64 view), made by the first SAM step
            # include/msig_wa.h: the weight-averaging shadow (parameters, BatchNorm state and counts), made by ensure_shadow()
            self.avg_params: Optional[torch.Tensor] = None
            self.avg_bn_state: Optional[torch.Tensor] = None
            self.avg_bn_count: Optional[torch.Tensor] = None
        else:
            self.params, self.grads = storage["params"], storage["grads"]
            self.bn_state, self.bn_count = storage["bn_state"], storage["bn_count"]
            self.exp_avg, self.exp_avg_sq = storage["exp_avg"], storage["exp_avg_sq"]
            self._ws_region = storage["ws"]
            self.loss_acc = storage["acc"]
            self.gc_state = storage.get("gc")
            if self.gc_state is not None:
                self.gc_state.zero_()
            self.sam_state = storage.get("sam")
            if self.sam_state is not None:
                self.sam_state.zero_()
            self.avg_params, self.avg_bn_state, self.avg_bn_count = (storage.get(k) for k in ("avg_params", "avg_bn_state", "avg_bn_count"))
            for t in (self.avg_params, self.avg_bn_state, self.avg_bn_count):
                if t is not None:
                    t.zero_()
            for t in (self.params, self.grads, self.exp_avg, self.exp_avg_sq, self.bn_state, self.bn_count, self.loss_acc):
                t.zero_()
        self.bn_state[16:32] = 1.0
        self.bn_state[64:96] = 1.0
        self.gru_layers = 2                     # msig_batch.gru_layers: EmbeddedEngine (the one-layer, 32-unit model) sets 1
        self._ws: Dict[Tuple[int, int, object], Tuple[torch.Tensor, list]] = {}
        self._ws_pool: Dict[object, torch.Tensor] = {}
        self._last: Optional[Tuple[int, int, object]] = None
        self._keep = None
        self._cw_checked = None                 # (weakref, version) of the last class-weight tensor whose values passed the checks
        self._st_key, self._st_desc = None, None  # the cached msig_st (`_st`)

    # ---- views -----------------------------------------------------------------
    def _numel(self, i):
        n = 1
        for s in self.shapes[i]:
            n *= s
        return n

    def param_view(self, i: int, flat: Optional[torch.Tensor] = None) -> torch.Tensor:
        flat = self.params if flat is None else flat
        o = self.layout[i]
        return flat[o:o + self._numel(i)].view(self.shapes[i])

    def named_param_views(self, flat: Optional[torch.Tensor] = None):
        """{state_dict key: view} of every parameter tensor of the model kind, in flat-buffer order."""
        return {k: self.param_view(i, flat) for i, k in self.keys}

    def bn_views(self):
        s = self.bn_state
        return {"cnn_encoder.1.running_mean": s[0:16], "cnn_encoder.1.running_var": s[16:32],
                "cnn_encoder.5.running_mean": s[32:64], "cnn_encoder.5.running_var": s[64:96],
                "cnn_encoder.1.num_batches_tracked": self.bn_count[0], "cnn_encoder.5.num_batches_tracked": self.bn_count[1]}

    def load_named(self, named: Dict[str, torch.Tensor]):
        """Copies a reference-style state_dict (any subset) into the flat buffers."""
        pv, bv = self.named_param_views(), self.bn_views()
        for k, v in named.items():
            dst = pv.get(k, bv.get(k))
            if dst is None:
                raise KeyError(k)
            dst.copy_(torch.as_tensor(v).to(dst.dtype).reshape(dst.shape))

    # ---- workspace ---------------------------------------------------------------
    EVAL_KEEP = "eval+keep"       # workspace mode of an eval forward kept for a backward (msig_batch.keep_for_backward)

    @classmethod
    def _mode(cls, training: bool, keep_for_backward: bool = False):
        """Workspace mode: True (training), False (evaluation) or EVAL_KEEP (evaluation kept for a backward: the training layout)."""
        return bool(training) or (cls.EVAL_KEEP if keep_for_backward else False)

    def workspace(self, B: int, T: int, training: bool, keep_for_backward: bool = False):
        mode = self._mode(training, keep_for_backward)
        key = (B, T, mode)
        if key not in self._ws:
            off = L.workspace_layout(B, self.C, T, self.K, mode is not False)
            if self._ws_region is not None:          # arena mode: every shape shares the arena's one workspace region
                if off[-1] > self._ws_region.numel():
                    raise RuntimeError(f"fold arena workspace too small for B={B}, T={T}")
                buf = self._ws_region[:off[-1]]
            else:
                # One allocation per mode, sized for the largest shape seen: the ragged last batch of an epoch lays its regions
                # out in the full batch's buffer instead of allocating a second one (13.6 GB each at B = 8192).  Training and
                # evaluation keep separate buffers — an evaluation between a training forward and its backward (autograd path)
                # must not overwrite the stash — and so does an evaluation kept for a backward (a third buffer, neither a pending
                # training forward's nor a plain evaluation's).  Growing frees the smaller buffer: layouts cached for it are dropped,
                # and a HIP graph captured on it must be re-captured (a graph holds raw pointers).
                pool = self._ws_pool.get(mode)
                if pool is None or pool.numel() < off[-1]:
                    for k in [k for k in self._ws if k[2] == mode]:
                        del self._ws[k]
                    if self._last is not None and self._last[2] == mode:
                        self._last, self._keep = None, None      # region() must not resolve to a purged layout
                    pool = None
                    self._ws_pool[mode] = pool = torch.empty(off[-1], dtype=torch.uint8, device=self.device)
                buf = pool[:off[-1]]
            lo = off[L.WS["LOSS"]]
            buf[lo:lo + 16].zero_()
            self._ws[key] = (buf, off)
        return self._ws[key]

    def drop_workspaces(self, mode=None):
        """Frees every workspace, or with `mode` (True, False or EVAL_KEEP) that mode's alone."""
        if mode is not None:
            for k in [k for k in self._ws if k[2] == mode]:
                del self._ws[k]
            self._ws_pool.pop(mode, None)
            if self._last is not None and self._last[2] == mode:
                self._last, self._keep = None, None
            return
        self._ws.clear()
        self._ws_pool.clear()
        self._last = None

    def region(self, name: str, dtype=torch.float32, shape=None, key=None) -> torch.Tensor:
        """A typed view of a workspace region of the last (or given) call."""
        key = key or self._last
        buf, off = self._ws[key]
        i = L.WS[name]
        raw = buf[off[i]:off[i + 1]].view(dtype)
        if shape is not None:
            n = 1
            for s in shape:
                n *= s
            raw = raw[:n].view(*shape)
        return raw

    # ---- descriptor ----------------------------------------------------------------
    def _batch(self, x: torch.Tensor, labels: Optional[torch.Tensor], training: bool, dropout_p: float,
               seed: int, step: int, keep_for_backward: bool = False) -> L.Batch:
        _require_gpu(x, "input batch")
        if x.dtype != torch.float32 or x.dim() != 3 or x.shape[1] != self.C:
            raise ValueError(f"expected float32 (B,{self.C},T) input, got {x.dtype} {tuple(x.shape)}")
        x = x.contiguous()
        B, _, T = x.shape
        if labels is not None:
            _require_gpu(labels, "labels")
            labels = labels.to(torch.int64).contiguous()
        keep = bool(keep_for_backward) and not training
        buf, off = self.workspace(B, T, training, keep)
        thr = L.dropout_threshold(dropout_p) if training else 0
        b = L.Batch()
        b.shape = L.Shape(B, self.C, T, self.K)
        b.training = int(training)
        b.keep_for_backward = int(keep)
        b.bn_momentum, b.bn_eps = 0.1, 1e-5
        b.dropout_thr = thr
        b.key_gru = L.dropout_key(seed, step, 1) if thr else 0
        b.key_head = L.dropout_key(seed, step, 2) if thr else 0
        b.x = x.data_ptr()
        b.labels = labels.data_ptr() if labels is not None else None
        b.params = self.params.data_ptr()
        b.grads = self.grads.data_ptr()
        b.bn_state = self.bn_state.data_ptr()
        b.bn_count = self.bn_count.data_ptr()
        b.ws = buf.data_ptr()
        b.ws_bytes = buf.numel()
        b.gru_layers = self.gru_layers
        b.loss_acc = self.loss_acc.data_ptr()
        L.apply_forms(b)
        self._last = (B, T, self._mode(training, keep))
        self._keep = (x, labels)
        return b

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _class_weight(self, w: Optional[torch.Tensor]) -> Optional[int]:
        """Device pointer of a class-weight vector (include/msig_cw.h) after the host-side checks — a contiguous (K,) float32 tensor
        on a GPU holding finite, non-negative values, else ValueError before anything is launched.  The values are read back once
        per tensor and version (an in-place change is seen), not once per step."""
        if w is None:
            return None
        _require_gpu(w, "class_weight")
        if w.dtype != torch.float32 or w.dim() != 1 or w.numel() != self.K or not w.is_contiguous():
            raise ValueError(f"class_weight must be a contiguous float32 ({self.K},) tensor, got {w.dtype} {tuple(w.shape)}")
        seen = self._cw_checked
        if seen is None or seen[0]() is not w or seen[1] != w._version:
            L.check_class_weight(w.detach().cpu().numpy(), self.K)
            self._cw_checked = (weakref.ref(w), w._version)
        return w.data_ptr()

    def _checked(self, class_weight, max_grad_norm, label_smoothing, mix_lambda):
        """The host-side checks of what forward() and train_step() take beyond the batch, before anything is scattered or launched
        (ValueError): (class-weight pointer or None, max_norm or None, smoothing, lam)."""
        return (self._class_weight(class_weight), None if max_grad_norm is None else L.check_max_grad_norm(max_grad_norm),
                L.check_label_smoothing(label_smoothing), L.check_mix_lambda(mix_lambda))

    def _st(self, cw: Optional[int], max_norm: Optional[float], smoothing: float, lam: float) -> L.St:
        """The msig_st of a call, with its msig_gc_clip when max_norm is given.  Cached under what determines it (the kind is the
        engine's): a step writes lam[0] and builds nothing.  The library reads a descriptor during the call, never after it."""
        state = None if max_norm is None else self.ensure_gc_state()
        key = (smoothing, cw, max_norm, None if state is None else state.data_ptr())
        if key != self._st_key:
            g = None
            if state is not None:
                g = L.GcClip()
                g.kind, g.class_weight, g.state, g.state_bytes = L.GC_KINDS[self.kind], cw, state.data_ptr(), state.numel() * 8
                g.max_norm[0] = max_norm
            self._st_key, self._st_desc = key, L.make_st(self.kind, smoothing, cw, g)
        self._st_desc.lam[0] = lam
        return self._st_desc

    # ---- calls -------------------------------------------------------------------------
    def forward(self, x, labels=None, training=False, dropout_p=0.0, seed=0, step=0, keep_for_backward=False,
                class_weight: Optional[torch.Tensor] = None, label_smoothing=0.0, mix_lambda=None, shadow: bool = False) -> L.Batch:
        """model(inputs) [+ criterion]: logits land in region('LOGITS'); returns the descriptor
        that a following backward() must be given.  An eval-mode forward (training=False) takes a backward only with
        keep_for_backward=True: it then keeps the stashes in a workspace of its own, with the same logits.  class_weight: a (K,)
        float32 device tensor = CrossEntropyLoss(weight=class_weight) for the loss and, kept for a backward, WS_DLOGITS
        (include/msig_cw.h); None = the unweighted criterion.  label_smoothing / mix_lambda: the soft-target criterion of
        include/msig_st.h — CrossEntropyLoss(label_smoothing=eps), and with mix_lambda = lam the loss against the
        row's own label (weight lam) and its partner's, row B-1-b (weight 1 - lam), for an `x` that was mixed the same way
        (mixup.Mixup.apply, DeviceLoader(mixup=)); 0.0 and None (or 1) = the plain criterion.
        shadow: an EVAL forward of the weight-averaging shadow (include/msig_wa.h) instead of the model — the same call with
        msig_batch.params / bn_state / bn_count pointing at it; the model's own buffers are not read."""
        cw, _, eps, lam = self._checked(class_weight, None, label_smoothing, mix_lambda)
        if shadow and (training or keep_for_backward):
            raise ValueError("the weight-averaging shadow takes eval-mode forwards only (training=False, keep_for_backward=False)")
        b = self._batch(x, labels, training, dropout_p, seed, step, keep_for_backward)
        if shadow:
            if self.avg_params is None:
                raise RuntimeError("this model has no weight-averaging shadow yet: call average_update first")
            b.params, b.bn_state, b.bn_count = self.avg_params.data_ptr(), self.avg_bn_state.data_ptr(), self.avg_bn_count.data_ptr()
        return self.forward_desc(b, cw, eps, lam)

    def forward_desc(self, b: L.Batch, cw: Optional[int] = None, smoothing: float = 0.0, lam: float = 1.0) -> L.Batch:
        """The forward of an already-built descriptor (`_batch`, possibly with pointers of it replaced: adapt.py, calibrate.py)."""
        L.check(L.lib().msig_st_forward(C.byref(b), C.byref(self._st(cw, None, smoothing, lam)), self._stream()), "msig_st_forward")
        return b

    def backward(self, b: L.Batch, dlogits: Optional[torch.Tensor] = None, dx: Optional[torch.Tensor] = None):
        """loss.backward() of the forward that returned `b`: parameter gradients into `grads`; with `dx` — a contiguous float32
        (B, C, T) tensor on this device — also dL/dx (msig_batch.dx)."""
        ptr = None
        if dlogits is not None:
            _require_gpu(dlogits, "dlogits")
            dlogits = dlogits.to(torch.float32).contiguous()
            ptr = dlogits.data_ptr()
        if dx is not None:
            _require_gpu(dx, "dx")
            if dx.dtype != torch.float32 or not dx.is_contiguous() or tuple(dx.shape) != (b.shape.B, self.C, b.shape.T):
                raise ValueError(f"dx must be a contiguous float32 ({b.shape.B}, {self.C}, {b.shape.T}) tensor, got {dx.dtype} {tuple(dx.shape)}")
            b = L.Batch.from_buffer_copy(b)          # the caller's descriptor stays as its forward left it
            b.dx = dx.data_ptr()
        if self.kind == "cnn_gru":
            L.check(L.lib().msig_cg_backward(C.byref(b), ptr, self._stream()), "msig_cg_backward")
        else:
            L.check(L.lib().msig_backward(C.byref(b), ptr, self._stream()), "msig_backward")

    def ensure_adam_state(self):
        if self.exp_avg is None:
            self.exp_avg = torch.zeros_like(self.params)
            self.exp_avg_sq = torch.zeros_like(self.params)

    def adam_step(self, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step=1):
        self.ensure_adam_state()
        L.check(L.lib().msig_adam_step(self.params.data_ptr(), self.grads.data_ptr(), self.exp_avg.data_ptr(),
                                       self.exp_avg_sq.data_ptr(), self.n_flat, lr, betas[0], betas[1], eps,
                                       weight_decay, step, self._stream()), "msig_adam_step")

    def ensure_gc_state(self) -> torch.Tensor:
        """The model's clip state (include/msig_gc.h): four float64 statistics, then the step's scratch."""
        if self.gc_state is None:
            self.gc_state = torch.zeros(L.gc_state_bytes(self.C, self.K, self.kind) // 8, dtype=torch.float64, device=self.device)
        return self.gc_state

    def zero_grad_stats(self):
        if self.gc_state is not None:
            self.gc_state[:L.GC_NSTAT].zero_()

    def grad_stats(self) -> Optional[dict]:
        """Gradient-norm statistics of the clipped steps since zero_grad_stats() (one read-back: a sync): sum, max and last of the
        norms before the clip, the number of steps and how many of them exceeded max_norm.  None before the first clipped step."""
        if self.gc_state is None:
            return None
        return self._stats(self.gc_state[:L.GC_NSTAT].cpu().tolist())

    @staticmethod
    def _stats(s) -> dict:
        return dict(sum=s[L.GC_SUM], max=s[L.GC_MAX], clipped=int(s[L.GC_CLIPPED]), last=s[L.GC_LAST])

    # ---- sharpness-aware minimisation (include/msig_sam.h) -------------------------------------------------------
    def ensure_sam_state(self) -> torch.Tensor:
        """The model's SAM state: L.SAM_NSTAT float64 statistics, then the step's scratch and backups."""
        if self.sam_state is None:
            self.sam_state = torch.zeros(L.sam_state_bytes(self.C, self.K, self.kind) // 8, dtype=torch.float64, device=self.device)
        return self.sam_state

    def zero_sam_stats(self):
        if self.sam_state is not None:
            self.sam_state[:L.SAM_NSTAT].zero_()

    def sam_stats(self) -> Optional[list]:
        """The SAM statistics since zero_sam_stats() as a list indexed by L.SAM_* (one read-back: a sync); None before the first SAM step."""
        return None if self.sam_state is None else self.sam_state[:L.SAM_NSTAT].cpu().tolist()

    def epoch_stats(self, grad: bool = False, sam: bool = False):
        """(loss_acc as a list, grad_stats() or None, sam_stats() or None) in ONE device-to-host copy: what a trainer reads at the end
        of an epoch."""
        parts = [self.loss_acc]
        if grad:
            parts.append(self.ensure_gc_state()[:L.GC_NSTAT])
        if sam:
            parts.append(self.ensure_sam_state()[:L.SAM_NSTAT])
        v = (torch.cat(parts) if len(parts) > 1 else parts[0]).cpu().tolist()
        g = self._stats(v[2:2 + L.GC_NSTAT]) if grad else None
        return v[:2], g, (v[-L.SAM_NSTAT:] if sam else None)

    def loss_and_grad_stats(self):
        """(loss_acc as a list, grad_stats()) in ONE device-to-host copy: what a trainer reads at the end of a clipped epoch."""
        return self.epoch_stats(grad=True)[:2]

    # ---- weight averaging (include/msig_wa.h) ------------------------------------------------------------------
    def ensure_shadow(self) -> torch.Tensor:
        """The model's shadow — avg_params, avg_bn_state, avg_bn_count — allocated (zeroed) at first use."""
        if self.avg_params is None:
            self.avg_params = torch.zeros_like(self.params)
            self.avg_bn_state = torch.zeros_like(self.bn_state)
            self.avg_bn_count = torch.zeros_like(self.bn_count)
        return self.avg_params

    def average_update(self, a: float) -> None:
        """One update of the shadow towards the model as it stands, shadow += a * (model - shadow) on every parameter and BatchNorm
        statistic in three fp32 roundings (msig_wa_update): a = 1 copies the model, a = 0 does nothing (no launch).  The
        coefficient is the caller's schedule (averaging.ema_coef / swa_coef); a number in [0, 1], else ValueError."""
        a = L.check_average_coef(a)
        self.ensure_shadow()
        w = L.Wa()
        w.n_flat, w.params, w.bn_state, w.bn_count = self.n_flat, self.params.data_ptr(), self.bn_state.data_ptr(), self.bn_count.data_ptr()
        w.avg_params, w.avg_bn_state, w.avg_bn_count = self.avg_params.data_ptr(), self.avg_bn_state.data_ptr(), self.avg_bn_count.data_ptr()
        w.coef[0] = a
        L.check(L.lib().msig_wa_update(C.byref(w), self._stream()), "msig_wa_update")

    def shadow_named(self) -> Dict[str, torch.Tensor]:
        """The shadow under the reference's state_dict keys (copies): every parameter tensor of the model kind, then the BatchNorm
        buffers in the order nn.Module.state_dict lists them."""
        if self.avg_params is None:
            raise RuntimeError("this model has no weight-averaging shadow yet: call average_update first")
        out = {k: v.clone() for k, v in self._shadow_param_views().items()}
        s, n = self.avg_bn_state, self.avg_bn_count
        out.update({"cnn_encoder.1.running_mean": s[0:16].clone(), "cnn_encoder.1.running_var": s[16:32].clone(),
                    "cnn_encoder.1.num_batches_tracked": n[0].clone(),
                    "cnn_encoder.5.running_mean": s[32:64].clone(), "cnn_encoder.5.running_var": s[64:96].clone(),
                    "cnn_encoder.5.num_batches_tracked": n[1].clone()})
        return out

    def _shadow_param_views(self) -> Dict[str, torch.Tensor]:
        return self.named_param_views(self.avg_params)

    def train_step(self, x, labels, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step=1,
                   dropout_p=0.0, seed=0, class_weight: Optional[torch.Tensor] = None, max_grad_norm: Optional[float] = None,
                   label_smoothing=0.0, mix_lambda=None, adversary=None, batch_index: Optional[torch.Tensor] = None, distill=None,
                   sam=None, dro=None, supcon=None) -> None:
        """optimizer.zero_grad(); loss = criterion(model(x), y); loss.backward(); optimizer.step()
        (trainer.py:144-149) as one asynchronous call; the batch loss is left in region('LOSS')[0] and added, times the batch size,
        to loss_acc[0] (loss_acc[1] += correctly classified windows): the caller zeroes loss_acc when an epoch starts.
        class_weight: (K,) float32 device tensor = criterion CrossEntropyLoss(weight=class_weight) (include/msig_cw.h).
        max_grad_norm: torch.nn.utils.clip_grad_norm_(model.parameters(), max_grad_norm) between loss.backward() and
        optimizer.step() (include/msig_gc.h): `grads` then holds the clipped gradient and grad_stats() the norms;
        float('inf') measures without clipping; None = unclipped.
        label_smoothing / mix_lambda: the soft-target criterion (include/msig_st.h; see forward()), with or without
        class weights and clip; 0.0 and None (or 1) = the plain criterion.
        adversary: an adversary.SubjectAdversary bound to this device (include/msig_da.h): one more launch trains it
        on the step's features and adds the reversed gradient of its loss, times its scheduled lambda, to the feature gradient; it
        advances its own step count.  batch_index: the int64 store positions of the rows (DeviceLoader.last_index) by which the
        adversary's domain table is read; None = the table has one entry per row.  The discriminator's Adam takes THIS call's betas,
        eps and weight_decay (L2 decay included) and lr * adversary.lr_mult.  None = no adversary.  One library call whatever is
        on (module docstring).
        distill: a distill.Distillation bound to this device (include/msig_kd.h): the head runs unfused and one more
        launch blends the gradient of the tempered KL term against the teacher rows — read by batch_index, or one per row — into
        the logits' gradient; the reported loss stays the criterion's, the term's own statistics go to distill.stats.  None, or
        alpha = 0, is the step without it, bit for bit.
        sam: a sam.Sam (include/msig_sam.h): the step runs twice over the batch — gradient at w, perturbation to
        w + e, gradient there with the same dropout masks, restore, Adam at w with the second gradient; `grads` holds that second
        gradient, region('LOSS') / loss_acc / the BatchNorm state are the first pass's, sam_stats() the norms and the sharpness.
        rho = 0 is the step without it, bit for bit.  Not with `adversary` (ValueError): two passes would advance the discriminator
        twice.  None = the step without it, exactly.
        dro: a dro.GroupDro bound to this device (include/msig_dro.h): the head runs unfused and one more launch
        moves the group weights dro.q with the groups' losses — groups read by batch_index, or one table entry per row — and
        rescales the logits' gradient so that the step descends sum_g q_g L_g; the reported loss stays the criterion's, the term's
        statistics go to dro.stats.  Under `sam` the weights move once, in the first pass.  Not with mixup (ValueError): a blended
        row has no group.  None = the step without it, exactly.
        supcon: a supcon.SupCon bound to this device (include/msig_sc.h): two more launches between the head's (the
        adversary's) and the GRU backward add weight x the gradient of the supervised contrastive loss on the step's features to
        the feature gradient — subjects read by batch_index, or one table entry per row, in cross-subject mode; the head stays fused
        where it was, the reported loss stays the criterion's, the term's statistics go to supcon.stats.  Under `sam` it runs in both
        passes.  weight = 0 measures and leaves the step its bits.  Not with mixup, not above 2048 windows (ValueError before any
        launch).  None = the step without it, exactly.
        Whatever is on, the step is ONE library call, msig_sc_train_step, with NULL for each term that is off (module docstring)."""
        cw, max_norm, smooth, lam = self._checked(class_weight, max_grad_norm, label_smoothing, mix_lambda)
        if supcon is not None:
            if lam != 1.0:
                raise ValueError("supcon cannot be combined with mixup: a row blended from two windows has no label to contrast")
            if x.shape[0] > min(L.SC_MAX_BATCH, supcon.max_batch or L.SC_MAX_BATCH):
                raise ValueError(f"supcon takes batches of at most {min(L.SC_MAX_BATCH, supcon.max_batch or L.SC_MAX_BATCH)} windows, got {x.shape[0]}")
            if supcon.cross_subject and batch_index is None and (supcon.grp is None or supcon.grp.numel() < x.shape[0]):
                raise ValueError(f"a subject table read by row needs {x.shape[0]} entries")
        if dro is not None:
            if lam != 1.0:
                raise ValueError("group-DRO cannot be combined with mixup: a row blended from two subjects has no group")
            if x.shape[0] > L.DRO_MAX_BATCH:
                raise ValueError(f"group-DRO takes batches of at most {L.DRO_MAX_BATCH} windows, got {x.shape[0]}")
            if batch_index is None and (dro.grp is None or dro.grp.numel() < x.shape[0]):
                raise ValueError(f"a group table read by row needs {x.shape[0]} entries")
        if sam is not None and adversary is not None:
            raise ValueError("sam cannot be combined with adversary: the discriminator's own Adam would advance in both passes")
        if adversary is not None and x.shape[0] > L.DA_MAX_BATCH:
            raise ValueError(f"subject-adversarial training takes batches of at most {L.DA_MAX_BATCH} windows, got {x.shape[0]}")
        if adversary is not None or distill is not None or dro is not None or supcon is not None:
            if batch_index is not None:
                _require_gpu(batch_index, "batch_index")
                if batch_index.dtype != torch.int64 or not batch_index.is_contiguous() or batch_index.numel() != x.shape[0]:
                    raise ValueError(f"batch_index must be a contiguous int64 ({x.shape[0]},) tensor, got {batch_index.dtype} {tuple(batch_index.shape)}")
        self.ensure_adam_state()
        b = self._batch(x, labels, True, dropout_p, seed, step)
        # the descriptors of the terms that are on, each built once; the library reads them during the call, never after it
        idx = None if batch_index is None else batch_index.data_ptr()
        a = k = sd = dd = cd = None
        if adversary is not None:
            adversary.last_lambda = adversary.next_lambda()
            a = adversary.descriptor([adversary.last_lambda], [lr * adversary.lr_mult], [adversary.step + 1], idx=idx, betas=betas, eps=eps,
                                     weight_decay=weight_decay)
        if distill is not None:
            if distill.q is None or distill.q.shape[1] != self.K or not distill.q.is_cuda or not distill.stats.is_cuda:
                raise ValueError(f"distill needs a (positions, {self.K}) teacher table bound to {self.device}: set_teacher, then bind")
            if batch_index is None and distill.q.shape[0] < x.shape[0]:
                raise ValueError(f"a teacher table read by row needs {x.shape[0]} rows, got {distill.q.shape[0]}")
            k = distill.descriptor(idx=idx)
        if sam is not None:
            state = self.ensure_sam_state()
            sd = sam.descriptor(self.kind, state.data_ptr(), state.numel() * 8)
        if dro is not None:
            dd = dro.descriptor(idx=idx)
        if supcon is not None:
            cd = supcon.descriptor(idx=idx)
        L.check(L.lib().msig_sc_train_step(C.byref(b), C.byref(self._st(cw, max_norm, smooth, lam)), _ref(a), _ref(k), _ref(sd), _ref(dd), _ref(cd),
                                           self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), lr, betas[0], betas[1], eps, weight_decay, step,
                                           self._stream()), "msig_sc_train_step")
        if adversary is not None:
            adversary.step += 1
        if adversary is not None or distill is not None or dro is not None or supcon is not None:
            self._keep = self._keep + (batch_index,)

    def features(self, x: torch.Tensor, padded: bool = False) -> torch.Tensor:
        """The (B, 128) vector the classifier sees, outputs[:, -1, :], of an EVAL-mode forward (running-statistics BatchNorm, no
        dropout, BatchNorm state untouched; msig_ft_features): front end and GRU, no head launch.  The rows are the bits an eval-mode
        forward() leaves in region('FEAT').  Leaves region() pointing at the call it pointed at before.  `padded` matters only to
        EmbeddedEngine."""
        last, keep = self._last, self._keep
        b = self._batch(x, None, False, 0.0, 0, 0)
        out = torch.empty((b.shape.B, 128), dtype=torch.float32, device=self.device)
        L.check(L.lib().msig_ft_features(C.byref(b), L.FT_KINDS[self.kind], out.data_ptr(), self._stream()), "msig_ft_features")
        if last is not None:
            self._last, self._keep = last, keep
        return out

    def stage(self, name: str, b: L.Batch):
        """Runs a single stage launcher by name (tests / profiling)."""
        fn = getattr(L.lib(), f"msig_{name}")
        if name == "head_ce_bwd":
            L.check(fn(C.byref(b), None, self._stream()), name)
        else:
            L.check(fn(C.byref(b), self._stream()), name)


def embedding_index(in_channels: int, num_classes: int, hidden: int = 32, kind: str = "cnn_gru_attention"):
    """The one-layer model's embedding in the padded 64-unit flat layout (EmbeddedEngine): ([(state_dict key, reference shape)]
    in flat-buffer order, int64 CPU index) — element i of the concatenated reference-shaped parameters lives at flat[index[i]]."""
    layout, shapes = L.param_layout(in_channels, num_classes, kind), L.param_shapes(in_channels, num_classes, kind)
    H = hidden
    small_shapes, idx = [], []
    gate_rows = torch.cat([torch.arange(g * 64, g * 64 + H) for g in range(3)])            # rows of the real units
    for i, k in L.param_keys(kind):
        o, shape = layout[i], shapes[i]
        if k.startswith("gru."):
            if "_l1" in k:
                continue                                            # no second layer in the embedded model
            if k.startswith("gru.weight_ih"):
                sm = (3 * H, shape[1]); ii = o + gate_rows[:, None] * shape[1] + torch.arange(shape[1])[None, :]
            elif k.startswith("gru.weight_hh"):
                sm = (3 * H, H); ii = o + gate_rows[:, None] * shape[1] + torch.arange(H)[None, :]
            else:
                sm = (3 * H,); ii = o + gate_rows
        elif k == "classifier.0.weight":                            # (64, 128): real features at columns 0..31 (forward) and 64..95 (reverse)
            cols = torch.cat([torch.arange(0, H), torch.arange(64, 64 + H)])
            sm = (shape[0], 2 * H); ii = o + torch.arange(shape[0])[:, None] * shape[1] + cols[None, :]
        else:
            n = 1
            for d in shape:
                n *= d
            sm, ii = tuple(shape), o + torch.arange(n)
        small_shapes.append((k, sm))
        idx.append(ii.reshape(-1).to(torch.int64))
    return small_shapes, torch.cat(idx)


class EmbeddedEngine(Engine):
    """The hierarchical experiment's second model (main.py:35-40: gru_hidden_size = 32, gru_num_layers = 1) on the kernels of the
    reference configuration.  Its GRU is embedded in layer 0 of the 64-unit layout: unit u of gate g sits at row g * 64 + u of the
    padded weight / bias tensors, every other row and column is zero.  A padded unit then has r = z = 1/2, n = 0, so its state stays
    exactly 0 from h_0 = 0, it feeds nothing into the real units (its W_hh columns multiply zeros), and its own weights receive exactly
    zero gradient (their gate gradients and its state are zero) — Adam with L2 decay keeps them at zero.  Layer 1 is skipped by the
    library (msig_batch.gru_layers = 1): outputs[:, -1, :] is layer 0's output at the last position, whose 64 + 64 columns hold the
    2 x 32 real features at columns 0..31 and 64..95 (classifier.0.weight is embedded the same way).

    The model's nn.Parameters are views of ONE contiguous buffer `small` (reference shapes, reference order); `index` maps its
    elements into the padded flat buffer.  scatter() / gather() move values between the two around every library call of a
    stand-alone model; in a fold batch's arena (FoldArena) only when a model enters, is checkpointed or is handed back."""

    def __init__(self, in_channels: int, num_classes: int, device: torch.device, hidden: int, storage: Optional[dict] = None,
                 kind: str = "cnn_gru_attention"):
        """`storage`: the padded buffers of one arena of a fold batch (FoldArena.engine).  The library then trains the padded layout
        in place; `small` is brought up to date (gather) and written back (scatter) only when the model's parameters are needed or
        replaced — checkpoints, evaluation, re-dealing — never per step."""
        super().__init__(in_channels, num_classes, device, storage, kind)
        if hidden != 32:
            raise NotImplementedError("embedded GRU: hidden size 32 (main.py:38)")
        self.gru_layers = 1
        self.hidden = hidden
        dev = self.device
        self.small_shapes, index = embedding_index(in_channels, num_classes, hidden, kind)
        self.index = index.to(dev)
        self.padding = torch.ones(self.n_flat, dtype=torch.bool, device=dev)   # entries of the flat buffer no model parameter maps to
        self.padding[self.index] = False
        self.small = torch.zeros(int(self.index.numel()), dtype=torch.float32, device=dev)
        self.small_grads = torch.zeros_like(self.small)

    def small_views(self, flat: Optional[torch.Tensor] = None):
        flat = self.small if flat is None else flat
        out, at = {}, 0
        for k, sm in self.small_shapes:
            n = 1
            for d in sm:
                n *= d
            out[k] = flat[at:at + n].view(sm)
            at += n
        return out

    def scatter(self):
        """model parameters -> padded flat buffer (the padding stays zero)."""
        self.params.zero_()
        self.params.index_copy_(0, self.index, self.small)

    def gather(self):
        self.small.copy_(self.params.index_select(0, self.index))

    def gather_grads(self):
        self.small_grads.copy_(self.grads.index_select(0, self.index))
        return self.small_views(self.small_grads)

    # ---- the library calls, with the embedding maintained around them ----
    def forward(self, x, labels=None, training=False, dropout_p=0.0, seed=0, step=0, keep_for_backward=False, class_weight=None,
                label_smoothing=0.0, mix_lambda=None, shadow=False):
        self._checked(class_weight, None, label_smoothing, mix_lambda)      # before the scatter: nothing runs on a bad argument
        self.scatter()
        return super().forward(x, labels, training, dropout_p, seed, step, keep_for_backward, class_weight, label_smoothing, mix_lambda, shadow)

    def average_update(self, a: float) -> None:
        """The shadow lives in the PADDED layout, like the buffers the library trains: the padding of a shadow that began as zeros
        or as a copy stays exactly +0.0 under the update (0 + a * (0 - 0) is exact).  shadow_named() gathers it to the
        reference-shaped tensors."""
        L.check_average_coef(a)
        self.scatter()
        super().average_update(a)

    def _shadow_param_views(self):
        return self.small_views(self.avg_params.index_select(0, self.index))

    def train_step(self, x, labels, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step=1, dropout_p=0.0, seed=0, class_weight=None,
                   max_grad_norm=None, label_smoothing=0.0, mix_lambda=None, adversary=None, batch_index=None, distill=None, sam=None,
                   dro=None, supcon=None):
        self._checked(class_weight, max_grad_norm, label_smoothing, mix_lambda)
        if sam is not None and adversary is not None:
            raise ValueError("sam cannot be combined with adversary: the discriminator's own Adam would advance in both passes")
        if adversary is not None:
            adversary.restrict_features(self.hidden)       # nothing may reach the padded feature columns (their units must stay zero)
        self.scatter()
        super().train_step(x, labels, lr, betas, eps, weight_decay, step, dropout_p, seed, class_weight, max_grad_norm, label_smoothing,
                           mix_lambda, adversary, batch_index, distill, sam, dro, supcon)
        self.gather()

    def features(self, x, padded: bool = False):
        """The one-layer model's real (B, 64) features: columns 0..31 (forward direction) and 64..95 (reverse) of the padded row;
        padded=True: the (B, 128) row itself, as the padded classifier.0.weight reads it (the other columns are exactly zero)."""
        self.scatter()
        f = super().features(x)
        if padded:
            return f
        return torch.cat([f[:, :self.hidden], f[:, 64:64 + self.hidden]], dim=1)

    def adam_step(self, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step=1):
        """Un-fused use: the caller has put the model's gradients into `small_grads` (MsigAdam.step)."""
        self.scatter()
        self.grads.zero_()
        self.grads.index_copy_(0, self.index, self.small_grads)
        super().adam_step(lr, betas, eps, weight_decay, step)
        self.gather()


def workspace_need(batch_sizes, in_channels: int, T: int, num_classes: int, training) -> int:
    """Bytes of a workspace that must serve every batch size in `batch_sizes` in one mode (allocates nothing).
    msig_workspace_layout is NOT monotonic in B — the projection region WS_GI exists only below 192 batch tiles, so a ragged last
    batch just under 3072 windows needs MORE than the full batch above it: from 192 tiles on, 191 tiles are a candidate too."""
    cand = {int(b) for b in batch_sizes}
    if max(cand) >= 192 * 16:
        cand.add(191 * 16)
    return max(L.workspace_layout(c, in_channels, T, num_classes, training)[-1] for c in cand)


def make_batch(B: int, C_: int, T: int, K: int, x: int, params: int, bn_state: int, bn_count: int, ws: int, ws_bytes: int, gru_layers: int,
               training: bool = False, dropout_thr: int = 0, labels: Optional[int] = None, grads: Optional[int] = None,
               loss_acc: Optional[int] = None) -> L.Batch:
    """msig_batch of B windows from device addresses: BatchNorm's constants, the binding's kernel forms, zero dropout keys (the
    *_multi calls carry their own), no keep_for_backward, no dx."""
    b = L.Batch()
    b.shape = L.Shape(B, C_, T, K)
    b.training = int(training)
    b.bn_momentum, b.bn_eps = 0.1, 1e-5
    b.dropout_thr = dropout_thr
    b.x, b.labels = x, labels
    b.params, b.grads = params, grads
    b.bn_state, b.bn_count = bn_state, bn_count
    b.ws, b.ws_bytes = ws, ws_bytes
    b.gru_layers = gru_layers
    b.loss_acc = loss_acc
    L.apply_forms(b)
    return b


def arena_layout(regions):
    """({name: (offset, nbytes)}, stride) of an arena that holds `regions`, an ordered (name, nbytes[, ...]) list, each at a
    256-byte-aligned offset.  Allocates nothing: tests/test_arena_layout_host.py pins the numbers."""
    off, at = {}, 0
    for name, nbytes, *_ in regions:
        off[name] = (at, nbytes)
        at += (nbytes + 255) // 256 * 256
    return off, at


class Arenas:
    """`n` identical arenas, `stride` bytes apart, in one zeroed allocation `mem` (n, stride): the regions of `regions`, an ordered
    (name, nbytes) list, at the same 256-byte-aligned offsets `off[name] = (offset, nbytes)` in each (`arena_layout`) — which is all a
    *_multi call needs to run the same work on several arenas in one set of launches."""
    form_folds = 1          # msig_multi.form_folds of multi(): the GRU backward form of ONE stand-alone fold (FoldArena.multi)

    def __init__(self, n: int, device, regions):
        self.n, self.device = int(n), torch.device(device)
        self.off, self.stride = arena_layout(regions)
        self.mem = torch.zeros((self.n, self.stride), dtype=torch.uint8, device=self.device)

    def view(self, slot: int, name: str, dtype=torch.uint8) -> torch.Tensor:
        o, nb = self.off[name]
        return self.mem[slot, o:o + nb].view(dtype)

    def ptr(self, name: str, slot: int = 0, byte_offset: int = 0) -> int:
        """Address of region `name` of arena `slot` (the *_multi calls are given arena 0's)."""
        return self.mem.data_ptr() + slot * self.stride + self.off[name][0] + byte_offset

    def across(self, name: str, byte_offset: int, dtype, count: int = 1) -> torch.Tensor:
        """(n, count) strided view of `count` elements at `byte_offset` inside region `name` of every arena."""
        o, _ = self.off[name]
        esz = torch.empty(0, dtype=dtype).element_size()
        flat = self.mem.view(dtype)                                    # (n, stride / esz)
        start = (o + byte_offset) // esz
        return flat[:, start:start + count]

    def stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def multi(self, slots, key_gru=None, key_head=None, lr=None, steps=None) -> L.Multi:
        m = L.Multi()
        m.n, m.stride_bytes, m.form_folds = len(slots), self.stride, self.form_folds
        for i, s in enumerate(slots):
            m.slot[i] = int(s)
            m.key_gru[i] = int(key_gru[i]) if key_gru is not None else 0
            m.key_head[i] = int(key_head[i]) if key_head is not None else 0
            m.lr[i] = float(lr[i]) if lr is not None else 0.0
            m.step[i] = int(steps[i]) if steps is not None else 0
        return m


class FoldArena(Arenas):
    """Device memory of a fold batch (include/msig.h msig_multi): `n` identical arenas, `stride` bytes apart, each holding one
    model's parameters, gradients, Adam moments, BatchNorm state, one workspace region, one input batch and its labels at the
    same offsets — which is all msig_*_multi needs to run the same step for several folds in one set of launches."""

    def __init__(self, in_channels: int, num_classes: int, device, n: int, train_batch: int, T: int, eval_batch: int = 0,
                 adaptive_forms: bool = False, gru_hidden: int = 64, gru_layers: int = 2, kind: str = "cnn_gru_attention",
                 grad_clip: bool = False, adversary: Optional[Tuple[int, int]] = None, averaging: bool = False,
                 distill: Optional[int] = None, sam: bool = False, dro: Optional[Tuple[int, int]] = None, supcon: Optional[int] = None):
        """(gru_hidden, gru_layers) = (32, 1): the arenas hold the one-layer model in EmbeddedEngine's padded 64-unit layout (params,
        grads and both Adam moments; the padding is written once, when a model enters its arena, and stays exactly zero), and every
        launch of the batch runs msig_batch.gru_layers = 1.  A fold batch is uniform in depth (msig_multi has no per-slot depth).
        `kind`: the model kind of every fold (Engine); it sizes the arenas from its layout.  A fold batch is uniform in kind too.
        `grad_clip`: the arenas also hold a "gc" region, each fold's clip state (include/msig_gc.h), after every other region —
        without it the arenas and their stride are what they are without this argument.
        `adversary` = (S, store positions), `distill` = store positions, `dro` = (G, store positions), `supcon` = store positions:
        every fold also gets the buffers of that optional step term — `side_regions` lists them — in a memory block of the term's
        own, an `Arenas` in `side[term]` with its own stride (`side_storage`, `side_stats`); the model arenas and their stride stay
        what they are without it.
        `averaging`: the arenas also hold every fold's weight-averaging shadow (include/msig_wa.h) — "avg_params", "avg_bn_state",
        "avg_bn_count" — after every other region, "gc" included: INSIDE the arenas, at the arena stride, because that is the only
        place the *_multi forward can read an averaged model from (`batch(..., shadow=True)`).  Without it the arenas and their
        stride are what they are without this argument.
        `sam`: the arenas also hold a "sam" region, each fold's SAM state (include/msig_sam.h), after every other region, the shadow
        included — without it the arenas and their stride are what they are without this argument."""
        if not (1 <= n <= L.MAX_FOLDS):
            raise ValueError(f"1..{L.MAX_FOLDS} folds per arena set")
        if (gru_hidden, gru_layers) not in ((64, 2), (32, 1)):
            raise NotImplementedError(f"fold arenas hold (gru_hidden, gru_layers) = (64, 2) or (32, 1), got {(gru_hidden, gru_layers)}")
        self.gru_hidden, self.gru_layers = int(gru_hidden), int(gru_layers)
        self.kind = L.check_kind(kind)
        eval_batch = int(eval_batch) or int(train_batch)
        self.C, self.K, self.T = in_channels, num_classes, T
        self.max_batch = max(int(train_batch), eval_batch)
        self.max_train_batch = int(train_batch)
        # The BACKWARD GRU kernel form is chosen as for ONE stand-alone fold of this batch size, whatever the number of folds in the
        # launch (form_folds = 1): a fold's bits must not depend on which companions share its launches, on when they stop early, on
        # --lockstep-groups or on how many ranks the folds are dealt to, and the backward forms round differently (they group the dW
        # partials differently).  adaptive_forms=True lets it follow the folds still active in each launch instead (msig.h: fused
        # backward kernels from 12 tiles per launch on).  The FORWARD forms are bit-identical since round 5: the library picks per
        # layer and per launch (gru.hip fwd_form) and this pin does not enter.
        self.adaptive_forms = bool(adaptive_forms)
        self.form_folds = 0 if self.adaptive_forms else 1
        self.n_flat = L.param_layout(in_channels, num_classes, kind)[-1]
        self.grad_clip, self.averaging, self.sam_on = bool(grad_clip), bool(averaging), bool(sam)
        self.max_norm = [float("inf")] * n              # per arena: max_norm of the fold in it (set_max_norm); inf = measured, not clipped
        side = self.side_regions(num_classes, train_batch, adversary, distill, dro, supcon)
        super().__init__(n, device, self.model_regions(in_channels, num_classes, T, train_batch, eval_batch, kind, self.grad_clip, self.averaging,
                                                       self.sam_on))
        self.ws_bytes = self.off["ws"][1]
        # the optional step terms: {term: (its memory block, `n` rows of its own stride; {region: dtype})} for the terms that are on
        self.side = {term: (Arenas(n, device, regs), {name: dt for name, _, dt in regs}) for term, regs in side.items()}
        self.dro_G = None if dro is None else int(dro[0])

    @classmethod
    def model_regions(cls, in_channels: int, num_classes: int, T: int, train_batch: int, eval_batch: int = 0, kind: str = "cnn_gru_attention",
                      grad_clip: bool = False, averaging: bool = False, sam: bool = False) -> list:
        """The ordered (name, nbytes) regions of one model arena (allocates nothing; `arena_layout` places them)."""
        n_flat = L.param_layout(in_channels, num_classes, kind)[-1]
        max_batch = max(int(train_batch), int(eval_batch) or int(train_batch))
        # "cw": the fold's class-weight vector (include/msig_cw.h msig_cw_*_multi), written when a fold enters (set_class_weight)
        sizes = [("params", n_flat * 4), ("grads", n_flat * 4), ("exp_avg", n_flat * 4), ("exp_avg_sq", n_flat * 4),
                 ("bn_state", L.BN_STATE_FLOATS * 4), ("bn_count", 16), ("acc", 16), ("x", max_batch * in_channels * T * 4), ("y", max_batch * 8),
                 ("ws", cls.workspace_bytes(train_batch, eval_batch, in_channels, T, num_classes)), ("cw", num_classes * 4)]
        if grad_clip:
            sizes.append(("gc", L.gc_state_bytes(in_channels, num_classes, kind)))
        if averaging:
            sizes += [("avg_params", n_flat * 4), ("avg_bn_state", L.BN_STATE_FLOATS * 4), ("avg_bn_count", 16)]
        if sam:
            sizes.append(("sam", L.sam_state_bytes(in_channels, num_classes, kind)))
        return sizes

    # constructor argument of each optional step term, as the "built without" error names it
    SIDE_ARGS = {"adversary": "adversary=(S, positions)", "distill": "distill=positions", "dro": "dro=(G, positions)", "supcon": "supcon=positions"}

    @staticmethod
    def side_regions(num_classes: int, train_batch: int, adversary=None, distill=None, dro=None, supcon=None) -> dict:
        """{term: ordered (name, nbytes, dtype) regions of one fold's row of the term's block} for the terms that are on, from the
        constructor's arguments (allocates nothing; `arena_layout` places them).  "stats" is every term's float64 statistics.
        adversary (include/msig_da.h): the discriminator's parameters, both Adam moments and an int32 domain table; distill
        (include/msig_kd.h): a teacher table of positions x K; dro (include/msig_dro.h): the weights q and an int32 group table;
        supcon (include/msig_sc.h): an int32 subject table and the scratch of a training batch."""
        f32, f64, i32 = torch.float32, torch.float64, torch.int32
        side = {}
        if adversary is not None:
            S, positions = int(adversary[0]), int(adversary[1])
            nf = L.da_param_floats(S)
            side["adversary"] = (("params", nf * 4, f32), ("exp_avg", nf * 4, f32), ("exp_avg_sq", nf * 4, f32), ("stats", 24, f64),
                                 ("dom", positions * 4, i32))
        if distill is not None:
            if int(distill) < 1:
                raise ValueError(f"distill takes the number of store positions (>= 1), got {distill!r}")
            side["distill"] = (("stats", 24, f64), ("q", int(distill) * num_classes * 4, f32))
        if dro is not None:
            G, positions = int(dro[0]), int(dro[1])
            if not 1 <= G <= L.DRO_MAX_GROUPS or positions < 1:
                raise ValueError(f"dro takes (groups in 1..{L.DRO_MAX_GROUPS}, store positions >= 1), got {dro!r}")
            side["dro"] = (("q", L.DRO_MAX_GROUPS * 4, f32), ("stats", L.DRO_STATS * 8, f64), ("grp", positions * 4, i32))
        if supcon is not None:
            if int(supcon) < 1 or int(train_batch) > L.SC_MAX_BATCH:
                raise ValueError(f"supcon takes the number of store positions (>= 1) and training batches of at most {L.SC_MAX_BATCH} "
                                 f"windows, got {supcon!r} and {train_batch}")
            side["supcon"] = (("stats", L.SC_STATS * 8, f64), ("grp", int(supcon) * 4, i32),
                              ("scratch", int(L.lib().msig_sc_scratch_bytes(int(train_batch))), torch.uint8))
        return side

    @staticmethod
    def workspace_bytes(train_batch: int, eval_batch: int, in_channels: int, T: int, num_classes: int) -> int:
        """Bytes of an arena's workspace region (allocates nothing): it serves training steps of at most `train_batch` windows and
        evaluation passes of at most `eval_batch` (the evaluation layout has no stash and no gradient scratch: a large
        --eval-batch-size must not be priced as a training batch): the maximum over every batch size that can occur
        (workspace_need)."""
        return max(workspace_need([train_batch], in_channels, T, num_classes, True),
                   workspace_need([int(eval_batch) or int(train_batch)], in_channels, T, num_classes, False))

    def engine(self, slot: int) -> Engine:
        st = {k: self.view(slot, k, torch.float32) for k in ("params", "grads", "exp_avg", "exp_avg_sq", "bn_state")}
        st["bn_count"] = self.view(slot, "bn_count", torch.int64)
        st["acc"] = self.view(slot, "acc", torch.float64)
        st["ws"] = self.view(slot, "ws")
        if self.grad_clip:
            st["gc"] = self.view(slot, "gc", torch.float64)
        if self.averaging:
            st["avg_params"], st["avg_bn_state"] = self.view(slot, "avg_params", torch.float32), self.view(slot, "avg_bn_state", torch.float32)
            st["avg_bn_count"] = self.view(slot, "avg_bn_count", torch.int64)
        if self.sam_on:
            st["sam"] = self.view(slot, "sam", torch.float64)
        if self.gru_layers == 1:
            return EmbeddedEngine(self.C, self.K, self.device, self.gru_hidden, storage=st, kind=self.kind)
        return Engine(self.C, self.K, self.device, storage=st, kind=self.kind)

    # ---- the optional step terms' side blocks: one table (`side`), one set of accessors -----------------------------------------------
    def _side(self, term: str) -> Arenas:
        if term not in self.side:
            raise RuntimeError(f"this FoldArena was built without {self.SIDE_ARGS[term]}: it has no {term} buffers")
        return self.side[term][0]

    def side_storage(self, term: str, slot: int) -> dict:
        """The buffers of `term` ("adversary", "distill", "dro", "supcon") of the fold in arena `slot`, what the term's object binds to
        (adversary.SubjectAdversary.bind, distill.Distillation.bind, dro.GroupDro.bind, supcon.SupCon.bind): typed views of its row."""
        blk = self._side(term)
        return {name: blk.view(slot, name, dt) for name, dt in self.side[term][1].items()}

    def side_stats(self, term: str) -> torch.Tensor:
        """(n, statistics) float64 strided view of every fold's statistics of `term`."""
        blk = self._side(term)
        return blk.across("stats", 0, torch.float64, blk.off["stats"][1] // 8)

    def zero_side_stats(self, term: str, slots) -> None:
        self.side_stats(term).index_fill_(0, torch.as_tensor(list(slots), dtype=torch.int64, device=self.device), 0.0)

    def da(self, slots, S: int, lambdas, lrs, steps, betas, eps, weight_decay) -> L.Da:
        """msig_da of a launch over `slots` (include/msig_da.h): fold slot 0's adversary buffers, the block's stride apart, and every
        fold's reversal weight, learning rate and step count.  idx / idx_row_stride are the launch's to fill in."""
        blk = self._side("adversary")
        a = L.Da()
        a.S, a.weight_decay, a.beta1, a.beta2, a.eps = int(S), weight_decay, betas[0], betas[1], eps
        a.dom, a.params, a.exp_avg, a.exp_avg_sq = blk.ptr("dom"), blk.ptr("params"), blk.ptr("exp_avg"), blk.ptr("exp_avg_sq")
        a.stats, a.stride_bytes = blk.ptr("stats"), blk.stride
        for i in range(len(slots)):
            getattr(a, "lambda")[i], a.lr[i], a.step[i] = float(lambdas[i]), float(lrs[i]), int(steps[i])
        return a

    def kd(self, alpha: float, temperature: float) -> L.Kd:
        """msig_kd of a launch (include/msig_kd.h): fold slot 0's teacher table and statistics, the block's stride apart.  idx /
        idx_row_stride are the launch's to fill in.  Checked on the host: ValueError before anything is launched."""
        blk = self._side("distill")
        k = L.Kd()
        k.alpha, k.temperature = L.check_distill(alpha, temperature)
        k.q, k.stats, k.stride_bytes = blk.ptr("q"), blk.ptr("stats"), blk.stride
        return k

    def dro(self, eta: float, frozen: bool = False) -> L.Dro:
        """msig_dro of a launch (include/msig_dro.h): fold slot 0's q, group table and statistics, the block's stride apart.  idx /
        idx_row_stride are the launch's to fill in."""
        blk = self._side("dro")
        d = L.Dro()
        d.G, d.eta, d.frozen = self.dro_G, float(eta), int(bool(frozen))
        d.q, d.grp, d.stats, d.stride_bytes = blk.ptr("q"), blk.ptr("grp"), blk.ptr("stats"), blk.stride
        return d

    def dro_stats(self) -> torch.Tensor:
        """(n, DRO_STATS + DRO_MAX_GROUPS) float64 copy of every fold's group-DRO statistics followed by its q (widened)."""
        return torch.cat([self.side_stats("dro"), self._side("dro").across("q", 0, torch.float32, L.DRO_MAX_GROUPS).to(torch.float64)], dim=1)

    def sc(self, positives: str, tau: float, weights) -> L.Sc:
        """msig_sc of a launch (include/msig_sc.h): fold slot 0's subject table, scratch and statistics, the block's stride apart, and
        the weight of every fold of the launch.  idx / idx_row_stride are the launch's to fill in (cross-subject mode)."""
        blk = self._side("supcon")
        d = L.Sc()
        d.positives, d.tau = L.SC_POSITIVES[positives], float(tau)
        d.grp = blk.ptr("grp") if d.positives else None
        d.scratch, d.stats, d.stride_bytes = blk.ptr("scratch"), blk.ptr("stats"), blk.stride
        for i, w in enumerate(weights):
            d.weight[i] = float(w)
        return d

    def set_class_weight(self, slot: int, values) -> None:
        """Writes the class-weight vector of the fold in arena `slot` (K values, checked on the host: ValueError before anything is
        written).  msig_cw_*_multi, given ptr("cw"), read fold z's vector in arena m.slot[z]; all ones = the unweighted criterion,
        bit for bit, so an unweighted fold can share launches with weighted ones."""
        w = L.check_class_weight(values, self.K)
        self.view(slot, "cw", torch.float32).copy_(torch.as_tensor(w, dtype=torch.float32))

    def set_max_norm(self, slot: int, value) -> None:
        """max_norm of the fold in arena `slot` (checked on the host: ValueError); float('inf') = its norms are measured, nothing is clipped."""
        if not self.grad_clip:
            raise RuntimeError("this FoldArena was built without grad_clip=True: it has no clip state")
        self.max_norm[slot] = L.check_max_grad_norm(value)

    def clip(self, slots, class_weight: Optional[int] = None) -> L.GcClip:
        """msig_gc_clip of a launch over `slots` (include/msig_gc.h): arena 0's clip state, every fold's own max_norm."""
        if not self.grad_clip:
            raise RuntimeError("this FoldArena was built without grad_clip=True: it has no clip state")
        g = L.GcClip()
        g.kind, g.class_weight, g.state, g.state_bytes = L.GC_KINDS[self.kind], class_weight, self.ptr("gc"), self.off["gc"][1]
        for i, s in enumerate(slots):
            g.max_norm[i] = self.max_norm[int(s)]
        return g

    def wa(self, slots, coefs) -> L.Wa:
        """msig_wa of a launch over `slots` (msig_wa_update_multi, include/msig_wa.h): arena 0's model and shadow buffers and the
        coefficient of every fold of the launch (checked on the host: ValueError before anything is launched)."""
        if not self.averaging:
            raise RuntimeError("this FoldArena was built without averaging=True: it has no shadow regions")
        if len(coefs) != len(slots):
            raise ValueError(f"{len(slots)} folds need {len(slots)} coefficients, got {len(coefs)}")
        w = L.Wa()
        w.n_flat, w.params, w.bn_state, w.bn_count = self.n_flat, self.ptr("params"), self.ptr("bn_state"), self.ptr("bn_count")
        w.avg_params, w.avg_bn_state, w.avg_bn_count = self.ptr("avg_params"), self.ptr("avg_bn_state"), self.ptr("avg_bn_count")
        for i, a in enumerate(coefs):
            w.coef[i] = L.check_average_coef(a)
        return w

    def soft(self, slots, smoothing: float, lams=None, class_weight: Optional[int] = None, clip: Optional[L.GcClip] = None) -> L.St:
        """msig_st of a launch over `slots` (msig_st_*_multi, include/msig_st.h): the launch's label smoothing, lam per fold of the
        launch (None: 1 everywhere — evaluation never mixes), ptr("cw") or None, and the launch's clip (`clip(slots)`) or None.
        Checked on the host: ValueError before anything is launched."""
        lams = [1.0] * len(slots) if lams is None else [L.check_mix_lambda(v) for v in lams]
        if len(lams) != len(slots):
            raise ValueError(f"{len(slots)} folds need {len(slots)} mixup weights, got {len(lams)}")
        return L.make_st(self.kind, L.check_label_smoothing(smoothing), class_weight, clip, lams)

    def sam(self, setting) -> L.Sam:
        """msig_sam of a launch (include/msig_sam.h) from a sam.Sam: arena 0's SAM state, the arena stride apart."""
        if not self.sam_on:
            raise RuntimeError("this FoldArena was built without sam=True: it has no SAM state")
        return setting.descriptor(self.kind, self.ptr("sam"), self.off["sam"][1])

    def zero_sam_stats(self, slots=None) -> None:
        st = self.across("sam", 0, torch.float64, L.SAM_NSTAT)
        if slots is None:
            st.zero_()
        else:
            st.index_fill_(0, torch.as_tensor(list(slots), dtype=torch.int64, device=self.device), 0.0)

    def zero_grad_stats(self, slots=None) -> None:
        st = self.across("gc", 0, torch.float64, L.GC_NSTAT)
        if slots is None:
            st.zero_()
        else:
            st.index_fill_(0, torch.as_tensor(list(slots), dtype=torch.int64, device=self.device), 0.0)

    def grad_stats(self, slot: int) -> dict:
        """Gradient-norm statistics of the fold in arena `slot` since zero_grad_stats (Engine.grad_stats; one read-back)."""
        return Engine._stats(self.view(slot, "gc", torch.float64)[:L.GC_NSTAT].cpu().tolist())

    def batch(self, B: int, training: bool, dropout_p: float, with_labels: bool = True, shadow: bool = False) -> L.Batch:
        """msig_batch describing arena 0 (the *_multi calls shift every pointer by slot * stride).  shadow: the eval descriptor that
        reads every fold's weight-averaging shadow instead of its model (params / bn_state / bn_count point at the "avg_*" regions)."""
        if shadow and (training or not self.averaging):
            raise ValueError("a shadow descriptor is an eval descriptor of a FoldArena built with averaging=True")
        if B > (self.max_train_batch if training else self.max_batch):
            raise ValueError(f"batch {B} exceeds the arena's {self.max_train_batch if training else self.max_batch}")
        model = ("avg_params", "avg_bn_state", "avg_bn_count") if shadow else ("params", "bn_state", "bn_count")
        return make_batch(B, self.C, self.T, self.K, self.ptr("x"), *(self.ptr(r) for r in model), self.ptr("ws"), self.ws_bytes, self.gru_layers,
                          training=training, dropout_thr=L.dropout_threshold(dropout_p) if training else 0,
                          labels=self.ptr("y") if with_labels else None, grads=self.ptr("grads"), loss_acc=self.ptr("acc"))

    def features(self, slots, B: int) -> torch.Tensor:
        """Eval-mode features (msig_ft_features_multi) of the B windows that sit in the "x" buffer of every arena in `slots`, in one
        set of launches: (len(slots), B, 128), or (len(slots), B, 64) — the real columns — for the one-layer model.  Fold z's rows are
        the bits Engine.features gives for the same model and windows."""
        out = torch.empty((len(slots), B, 128), dtype=torch.float32, device=self.device)
        b, m = self.batch(B, False, 0.0, with_labels=False), self.multi(slots)
        L.check(L.lib().msig_ft_features_multi(C.byref(b), C.byref(m), L.FT_KINDS[self.kind], out.data_ptr(), B * 512, self.stream()),
                "msig_ft_features_multi")
        if self.gru_layers == 1:
            return torch.cat([out[:, :, :self.gru_hidden], out[:, :, 64:64 + self.gru_hidden]], dim=2)
        return out
