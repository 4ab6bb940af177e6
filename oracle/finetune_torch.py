"""CPU oracle (TEST INFRASTRUCTURE ONLY) for SURVEY row N2: the trainable head of the CLIP multi-scale adapter
fine-tune step, restated in torch (float64 by default) with autograd for the gradients.

Follows /root/reference/finetune_module/clip_multiscale_adapter.py:
  * encode_image :134-149  -- per-block CLS features (detached by the hooks, utils.py:6-18) -> bias-free Linear ->
                              concat with the CLIP image feature -> res*f + (1-res)*AdapterMLP(f) -> F.normalize
                              (note: here res weights the ORIGINAL feature, the opposite of ARPDT.py:466-472)
  * encode_text  :151-175  -- same on the EOT-token features of the text tower
  * forward      :177-250  -- VIP loss (:214-220; `r` is [B,1] and the scores are [B], so the exponent BROADCASTS to a
                              [B,B] matrix before the mean -- kept), inverse-dynamics CE on concat[a1,t,a2,t] (:232-237),
                              total = vip + lambda_id * id with lambda_id a learnable scalar used as is (:103,246)
  * AdapterMLP   layers.py:6-60 with num_layers = 2: Linear -> Identity -> ReLU -> Linear
and finetune.py:139-141 for the optimiser: CLIP frozen, torch.optim.AdamW(lr, weight_decay) over everything else.

Pinned by tests/golden/finetune_tiny.npz: outputs and gradients of the REFERENCE CLASS ITSELF executed in the build
container on a stub CLIP (tests/golden/make_golden_finetune.py).  The reference has no tests of its own for this
path: parity unpinned by the reference beyond that fixture.

`Rounding` (operand="f16" / "bf16" in forward / grads) is a second, TEST-ONLY reading of the same head: still float64, but rounded
(round-to-nearest-even) to the 16-bit operand type exactly where arp_amd/csrc/arp_ft.hip rounds in its 16-bit modes, with the
backward seeded x grad_scale as the f16 mode seeds it.  The default (operand=None) runs the plain code above, unchanged.
"""
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F


@dataclass
class HeadConfig:
    layers: int = 12        # CLIP blocks whose CLS / EOT features are concatenated (clip_model.transformer.layers)
    width_v: int = 768      # vision tower width
    width_t: int = 512      # text tower width (= embed = input_dim = output_dim in the reference's constructor defaults)
    embed: int = 512
    hidden: int = 1024      # hidden_dim; the adapters use hidden*(layers+1), the inverse model uses hidden
    n_actions: int = 15
    gamma: float = 0.98
    logit_scale: float = float(np.log(1 / 0.07))
    use_vip: bool = True
    use_id: bool = True
    goal_conditioned: bool = False  # clip_multiscale_adapter.py:208-212,224-230: image3 stands where the prompt stands

    @property
    def d_img(self):
        return self.layers * self.width_v

    @property
    def d_txt(self):
        return self.layers * self.width_t

    @property
    def feat(self):
        return self.layers * self.width_t + self.embed

    @property
    def adapter_hidden(self):
        return self.hidden * (self.layers + 1)


def param_shapes(cfg):
    """torch state_dict names of CLIPMultiscaleAdapter without clip_model.* (Linear weights are [out, in])."""
    Fd, Hd = cfg.feat, cfg.adapter_hidden
    s = {"image_intermediate_linear.weight": (cfg.d_txt, cfg.d_img), "text_intermediate_linear.weight": (cfg.d_txt, cfg.d_txt)}
    for a in ("image_adapter", "text_adapter"):
        s[f"{a}.layers.0.weight"] = (Hd, Fd)
        s[f"{a}.layers.0.bias"] = (Hd,)
        s[f"{a}.layers.3.weight"] = (Fd, Hd)
        s[f"{a}.layers.3.bias"] = (Fd,)
    s["inverse_layer.layers.0.weight"] = (cfg.hidden, 4 * Fd)
    s["inverse_layer.layers.0.bias"] = (cfg.hidden,)
    s["inverse_layer.layers.3.weight"] = (cfg.n_actions, cfg.hidden)
    s["inverse_layer.layers.3.bias"] = (cfg.n_actions,)
    s["image_residual_weight"] = ()
    s["text_residual_weight"] = ()
    s["lambda_id"] = ()
    return s


def init_params(cfg, seed=0, scale=1.0):
    """Seeded stand-in init (the reference uses orthogonal weights, zero biases, 4.0 residual weights, lambda_id = ln(1/0.07))."""
    rng = np.random.Generator(np.random.PCG64(seed))
    P = {}
    for k, shp in param_shapes(cfg).items():
        if k.endswith("residual_weight"):
            P[k] = np.float32(4.0) + np.zeros(shp, np.float32)
        elif k == "lambda_id":
            P[k] = np.float32(np.log(1 / 0.07)) + np.zeros(shp, np.float32)
        elif k.endswith(".bias"):
            P[k] = (0.02 * rng.standard_normal(shp)).astype(np.float32)
        else:
            P[k] = (scale * rng.standard_normal(shp) / np.sqrt(shp[1])).astype(np.float32)
    return P


class _RoundValue(torch.autograd.Function):
    """forward: RNE to the operand type; backward: the gradient passes unchanged (the f32 dX product reads the rounded operand)."""

    @staticmethod
    def forward(ctx, x, rq, sat):
        return rq.q(x, sat)

    @staticmethod
    def backward(ctx, g):
        return g, None, None


class _RoundGrad(torch.autograd.Function):
    """forward: identity; backward: the incoming gradient is rounded to the operand type (a 16-bit gradient operand)."""

    @staticmethod
    def forward(ctx, x, rq, point, sat):
        ctx.rq, ctx.point, ctx.sat = rq, point, sat
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        q = ctx.rq.q(g, ctx.sat)
        ctx.rq.record(ctx.point, q)
        return q, None, None, None


class _ReluRound(torch.autograd.Function):
    """H = T(relu(x)) (a GEMM epilogue: past binary16's range it is inf); backward: the STORED activation masks the incoming 16-bit dH
    and the masked copy saturates, as transpose_mask_kernel does (mask > 0 ? dH : 0)."""

    @staticmethod
    def forward(ctx, x, rq):
        y = rq.q(F.relu(x), sat=False)
        ctx.save_for_backward(y)
        ctx.rq = rq
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        return torch.where(y > 0, ctx.rq.saturate(g), torch.zeros_like(g)), None


class Rounding:
    """Where arp_ft.hip's 16-bit modes (T = binary16 / bfloat16) round, for the float64 emulation.  Each point can be switched off
    (`skip`, for the tests that prove every point fires); `trace` (a dict) collects what each point produced.
      forward   "x"       tower features X -> T                          "weights" Wint, W1, W2, V1 read from the T mirror
                "f"       f = [X Wint^T | final] -> T as fc1's operand    "H"       relu(f W1^T + b1) stored as T
                "C"       C = [a1 | t | a2 | t] -> T
      backward  "dHinv"   relu-masked dlogits V2 -> T (dc1 = its row sum, dV1 = dHinv^T C, dC = dHinv V1)
                "dA"      dA -> T for dW2 and dH (db2 = the column sum of the f32 dA)
                "dH"      dA W2 -> T, then masked by H > 0 (db1 = row sum, dW1, and dHp W1 into the f32 df)
                "dU"      df[:, :Dt] -> T for dWint
    Everything else (U, A, the mix / normalise, the scores, Hinv, the logits, V2 / c2, the scalars) is f32 on the GPU: plain float64
    here.  The backward is seeded x grad_scale (1024 in f16, as ft_loss_kernel seeds it; 1 in bf16): the points round scale * value.
    Range as on the GPU: in f16 the f32 -> T copies (transpose_mask_kernel: x, f, C, dHinv, dA, dU, and the masked dH) saturate at
    +-65504; the GEMM epilogues that store T (H, dH) and the weight mirror overflow to inf."""

    POINTS = ("x", "weights", "f", "H", "C", "dHinv", "dA", "dH", "dU")
    SATURATE = ("x", "f", "C", "dHinv", "dA", "dU")

    def __init__(self, operand, grad_scale=None, skip=(), trace=None):
        self.dtype = {"f16": torch.float16, "bf16": torch.bfloat16}[operand]
        self.grad_scale = float(grad_scale if grad_scale is not None else (1024.0 if operand == "f16" else 1.0))
        self.skip = frozenset(skip)
        assert self.skip <= set(self.POINTS), self.skip
        self.trace = trace

    def saturate(self, x):
        return x.clamp(-65504.0, 65504.0) if self.dtype == torch.float16 else x  # (NaN stays NaN)

    def q(self, x, sat):
        return (self.saturate(x) if sat else x).to(self.dtype).to(x.dtype)

    def record(self, point, v):
        if self.trace is not None:
            self.trace.setdefault(point, []).append(v.detach())

    def value(self, point, x):
        if point in self.skip:
            return x
        y = _RoundValue.apply(x, self, point in self.SATURATE)
        self.record(point, y)
        return y

    def grad(self, point, x):
        return x if point in self.skip else _RoundGrad.apply(x, self, point, point in self.SATURATE)

    def relu(self, point, x):
        if point in self.skip:
            return F.relu(x)
        y = _ReluRound.apply(x, self)
        self.record(point, y)
        return y


def _adapter(P, name, x, rq=None):
    if rq is None:
        h = F.relu(F.linear(x, P[f"{name}.layers.0.weight"], P[f"{name}.layers.0.bias"]))
        return F.linear(h, P[f"{name}.layers.3.weight"], P[f"{name}.layers.3.bias"])
    h = rq.grad("dH", rq.relu("H", F.linear(rq.value("f", x), rq.value("weights", P[f"{name}.layers.0.weight"])) + P[f"{name}.layers.0.bias"]))
    return rq.grad("dA", F.linear(h, rq.value("weights", P[f"{name}.layers.3.weight"]))) + P[f"{name}.layers.3.bias"]


def _encode(P, which, inter, final, rq=None):
    if rq is None:
        u = F.linear(inter, P[f"{which}_intermediate_linear.weight"])
    else:
        u = rq.grad("dU", F.linear(rq.value("x", inter), rq.value("weights", P[f"{which}_intermediate_linear.weight"])))
    f = torch.cat([u, final], dim=-1)
    res = torch.sigmoid(P[f"{which}_residual_weight"])
    y = res * f + (1.0 - res) * _adapter(P, f"{which}_adapter", f, rq)
    return F.normalize(y, dim=-1)


def forward(P, cfg, img_inter, img_final, txt_inter, txt_final, r, action, rq=None):
    """img_inter [3,B,d_img], img_final [3,B,embed] (frames 0,1,2 of each sample), txt_inter [B,d_txt], txt_final [B,embed],
    r [B] as stored in the batch (the loss uses r - 1), action [B] int64.  goal_conditioned: FOUR image groups, txt_* = None.
    rq: a Rounding (the 16-bit emulation) or None (the plain oracle)."""
    a = [_encode(P, "image", img_inter[k], img_final[k], rq) for k in range(3)]
    if cfg.goal_conditioned:
        # :208-212 -- img_inter / img_final carry FOUR groups (image0..image3); the scores are negative distances to the goal frame's
        # adapted feature, which also takes the prompt's two slots of the inverse-model input (:224-230); no text tower, no logit scale
        t = _encode(P, "image", img_inter[3], img_final[3], rq)
        s = [-torch.linalg.norm(t - a[k], dim=-1) for k in range(3)]
    else:
        t = _encode(P, "text", txt_inter, txt_final, rq)
        scale = float(np.exp(cfg.logit_scale))
        s = [scale * (a[k] * t).sum(-1) for k in range(3)]
    rr = (r - 1.0).reshape(-1, 1)  # [B,1] against [B] scores: a [B,B] exponent, exactly as the reference broadcasts
    vip = (1 - cfg.gamma) * -s[0].mean() + torch.log(1e-8 + torch.mean(torch.exp(-(rr + cfg.gamma * s[2] - s[1]))))
    c = torch.cat([a[1], t, a[2], t], dim=-1)
    if rq is None:
        h = F.relu(F.linear(c, P["inverse_layer.layers.0.weight"], P["inverse_layer.layers.0.bias"]))
    else:
        h = F.relu(rq.grad("dHinv", F.linear(rq.value("C", c), rq.value("weights", P["inverse_layer.layers.0.weight"])) + P["inverse_layer.layers.0.bias"]))
    logits = F.linear(h, P["inverse_layer.layers.3.weight"], P["inverse_layer.layers.3.bias"])
    idl = F.cross_entropy(logits, action)
    loss = 0.0
    if cfg.use_vip:
        loss = loss + vip
    if cfg.use_id:
        loss = loss + P["lambda_id"] * idl
    return {"loss": loss, "vip_loss": vip, "id_loss": idl, "scores": torch.stack(s), "logits": logits, "adapted_image": torch.stack(a),
            "adapted_text": t}


def to_torch(P, dtype=torch.float64, requires_grad=False):
    return {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=requires_grad) for k, v in P.items()}


def grads(P, cfg, batch, dtype=torch.float64, operand=None, grad_scale=None, skip=(), trace=None):
    """d loss / d every parameter.  operand = "f16" / "bf16": the rounded-operand emulation of arp_ft.hip's 16-bit mode (Rounding), its
    backward seeded x grad_scale (default: the mode's own, 1024 / 1) and the gradients divided by it again, as arp_ft_get_tensor does."""
    Pt = to_torch(P, dtype, requires_grad=True)
    rq = None if operand is None else Rounding(operand, grad_scale, skip, trace)
    out = forward(Pt, cfg, *[None if b is None else torch.as_tensor(b, dtype=dtype) for b in batch[:5]], torch.as_tensor(batch[5], dtype=torch.long),
                  **({} if rq is None else {"rq": rq}))
    if rq is None:
        out["loss"].backward()
    else:
        out["loss"].backward(torch.tensor(rq.grad_scale, dtype=dtype))
        for v in Pt.values():
            if v.grad is not None:
                v.grad /= rq.grad_scale
    g = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach().numpy() for k, v in Pt.items()}
    aux = {k: float(out[k].detach()) for k in ("loss", "vip_loss", "id_loss")}
    aux["scores"], aux["logits"] = out["scores"].detach().numpy(), out["logits"].detach().numpy()
    aux["no_grad"] = tuple(k for k, v in Pt.items() if v.grad is None)  # torch.optim.AdamW leaves these untouched
    return g, aux


def adamw_step(P, M, V, G, step, lr, weight_decay, b1=0.9, b2=0.999, eps=1e-8, no_grad=()):
    """torch.optim.AdamW semantics (decoupled decay on every parameter THAT HAS A GRADIENT -- one whose .grad is None is skipped
    entirely: no decay, no moment update -- bias correction with t = step + 1)."""
    t = step + 1
    out_p, out_m, out_v = {}, {}, {}
    for k in P:
        if k in no_grad:
            out_p[k], out_m[k], out_v[k] = np.asarray(P[k], np.float64), M[k], V[k]
            continue
        p = np.asarray(P[k], np.float64) * (1.0 - lr * weight_decay)
        m = b1 * np.asarray(M[k], np.float64) + (1 - b1) * G[k]
        v = b2 * np.asarray(V[k], np.float64) + (1 - b2) * G[k] * G[k]
        denom = np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps
        out_p[k] = p - (lr / (1 - b1 ** t)) * m / denom
        out_m[k], out_v[k] = m, v
    return out_p, out_m, out_v


def train_steps(P, cfg, batches, lr, weight_decay, n_steps):
    M = {k: np.zeros_like(np.asarray(v, np.float64)) for k, v in P.items()}
    V = {k: np.zeros_like(np.asarray(v, np.float64)) for k, v in P.items()}
    P = {k: np.asarray(v, np.float64) for k, v in P.items()}
    aux = []
    for i in range(n_steps):
        g, a = grads(P, cfg, batches[i % len(batches)])
        aux.append(a)
        P, M, V = adamw_step(P, M, V, g, i, lr, weight_decay, no_grad=a["no_grad"])
    return P, aux
