"""Oracle (test infrastructure): the InstructRL baseline policy (/root/reference/arp_dt/BC.py, built by main_procgen.py:406-427 when
use_vl=False and vl_type="BC") restated in torch, fp64; autograd supplies the backward.  The ARP-DT oracle (oracle/arpdt_torch.py)
is left as it is; this module restates what BC changes and reuses its configuration, ALiBi slopes and state layout.

Against ARPDT.py, for the shipped configuration (m3ae encodings in, use_adapter=True, use_discrete_action=True, one image key,
no state input, num_obs_token = 1):

  * adapter MLP + residual mix, image_text_input + tanh ... BC.py:322-343 (as ARPDT.py:462-484)
  * NO rtg_input, NO return_outputs_* ..................... BC.py:87-100 (the parameter tree is ARP-DT's minus those)
  * tokens [image, action] per time step, L = 2T ........... BC.py:141-147
  * the vit_* custom mask at num_obs_token = 1 is the plain causal mask (the block diagonal of 1x1 ones adds nothing) .. BC.py:149-163
  * action head on the image-token rows 0::2 ................ BC.py:164-175 ((num_obs_token - 1) :: num_token_per_step)
  * loss = the cross-entropy over all B*T*n_actions elements, acc; output {action_pred, loss, acc} .. BC.py:177-181,230-241
  * aux of create_train_step / create_val_step: trans_loss = return_loss = 0.0 (output.get(..., 0.0)) .. main_procgen.py:118-124,153-157
  * L2 term, pmean, clip_by_global_norm, adamw with the all-False decay mask ........ main_procgen.py:105-139,490-507
    (restated as oracle/arpdt_torch.py:176-205 does)
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import arpdt_torch as O

PolicyConfig = O.PolicyConfig  # lambda_ret is not read: BC has no return loss
init_state = O.init_state


def param_shapes(cfg):
    """ARP-DT's Flax tree without rtg_input/kernel and return_outputs_0/* (BC.py:87-100)."""
    return {k: v for k, v in O.param_shapes(cfg).items() if not (k == "rtg_input/kernel" or k.startswith("return_outputs_0/"))}


def num_params(cfg):
    return int(sum(np.prod(v) for v in param_shapes(cfg).values()))


def forward(P, cfg, enc, action):
    """P: dict name -> tensor.  enc [B,T,tokens,dim], action int64 [B,T].  Returns dict(action_pred [B,T,n_actions], loss, acc)."""
    B, T = action.shape
    E = cfg.emb
    x = enc.reshape(B * T * cfg.enc_tokens, cfg.enc_dim)
    if cfg.use_adapter:
        a = F.relu(x @ P["AdapterMLP_0/Dense_0/kernel"] + P["AdapterMLP_0/Dense_0/bias"])
        a = F.relu(a @ P["AdapterMLP_0/Dense_1/kernel"] + P["AdapterMLP_0/Dense_1/bias"])
        res = torch.sigmoid(P["residual_weight"])
        x = res * a + (1 - res) * x
    img = torch.tanh(x.reshape(B, T, -1) @ P["image_text_input/kernel"] + P["image_text_input/bias"])
    act = P["action_input/embedding"][action]
    tok = torch.cat([img, act], dim=-1).reshape(B, 2 * T, E)
    L = 2 * T
    mask = torch.tril(torch.ones(L, L, dtype=torch.bool, device=tok.device))
    hd = E // cfg.heads
    h = tok
    for i in range(cfg.depth):
        p = f"policy/Block_{i}/"
        y = F.layer_norm(h, (E,), P[p + "LayerNorm_0/scale"], P[p + "LayerNorm_0/bias"], 1e-6)
        qkv = y @ P[p + "Attention_0/Dense_0/kernel"] + P[p + "Attention_0/Dense_0/bias"]
        q, k, v = (t.reshape(B, L, cfg.heads, hd).transpose(1, 2) for t in qkv.split(E, dim=-1))
        att = (q @ k.transpose(-2, -1)) * hd ** -0.5
        if getattr(cfg, "alibi_bias", False):
            sl = torch.tensor(O.alibi_slopes(cfg.heads), dtype=att.dtype, device=att.device)
            att = att + sl[None, :, None, None] * torch.arange(L, dtype=att.dtype, device=att.device)[None, None, None, :]
        att = att.masked_fill(~mask, torch.finfo(att.dtype).min).softmax(-1)
        y = (att @ v).transpose(1, 2).reshape(B, L, E)
        h = h + y @ P[p + "Attention_0/Dense_1/kernel"] + P[p + "Attention_0/Dense_1/bias"]
        y = F.layer_norm(h, (E,), P[p + "LayerNorm_1/scale"], P[p + "LayerNorm_1/bias"], 1e-6)
        y = F.gelu(y @ P[p + "FeedForward_0/fc1/kernel"], approximate="tanh") @ P[p + "FeedForward_0/fc2/kernel"]
        h = h + y
    h = F.layer_norm(h, (E,), P["policy/LayerNorm_0/scale"], P["policy/LayerNorm_0/bias"], 1e-6)
    a_in = h[:, 0::2]  # (num_obs_token - 1) :: num_token_per_step with num_obs_token = 1, 2 tokens per step
    n = "action_outputs_0"
    logits = F.relu(a_in @ P[n + "/layers_0/kernel"] + P[n + "/layers_0/bias"]) @ P[n + "/layers_2/kernel"]
    onehot = F.one_hot(action, cfg.n_actions).to(logits.dtype)
    loss = (-onehot * F.log_softmax(logits, -1)).mean()
    acc = (logits.argmax(-1) == action).to(logits.dtype).mean()
    return dict(action_pred=logits, loss=loss, acc=acc)


def loss_and_aux(P, cfg, enc, action):
    """loss_fn of create_train_step (main_procgen.py:105-126) around BC: trans_loss / return_loss are absent from the output -> 0.0."""
    out = forward(P, cfg, enc, action)
    l2 = sum((p ** 2).sum() for p in P.values() if p.ndim > 1)
    pen = cfg.weight_decay * 0.5 * l2
    loss = out["loss"] + pen
    aux = dict(loss=loss, acc=out["acc"] * 100, trans_loss=0.0, return_loss=0.0, weight_penalty=pen, weight_l2=l2)
    return loss, aux, out


def val_aux(P, cfg, enc, action):
    """val_fn of create_val_step (main_procgen.py:145-160)."""
    out = forward(P, cfg, enc, action)
    return dict(loss=float(out["loss"]), trans_loss=0.0, return_loss=0.0, acc=float(out["acc"]) * 100)


def grads(P, cfg, enc, action):
    Pr = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    loss, aux, out = loss_and_aux(Pr, cfg, enc, action)
    loss.backward()
    g = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in Pr.items()}
    return g, {k: float(v.detach()) if torch.is_tensor(v) else float(v) for k, v in aux.items()}, {k: v.detach() for k, v in out.items()}


def train_step(state, cfg, shards, lr_fn):
    """One reference train step on a list of per-device (enc, action) shards: pmean, clip_by_global_norm, adam with decoupled decay
    masked off (main_procgen.py:128-139,490-507; the update of oracle/arpdt_torch.py:train_step)."""
    P = state["params"]
    gs, auxs = [], []
    for enc, action in shards:
        g, aux, _ = grads(P, cfg, enc, action)
        gs.append(g)
        auxs.append(aux)
    n = len(shards)
    g = {k: sum(gi[k] for gi in gs) / n for k in P}
    aux = {k: sum(a[k] for a in auxs) / n for k in auxs[0]}
    gnorm = torch.sqrt(sum((v ** 2).sum() for v in g.values()))
    if gnorm >= cfg.clip_norm:
        g = {k: v / gnorm * cfg.clip_norm for k, v in g.items()}
    step = state["step"]
    lr = float(lr_fn(step))
    t = step + 1
    new = dict(params={}, mu={}, nu={}, step=t)
    for k in P:
        mu = cfg.b1 * state["mu"][k] + (1 - cfg.b1) * g[k]
        nu = cfg.b2 * state["nu"][k] + (1 - cfg.b2) * g[k] ** 2
        mhat = mu / (1 - cfg.b1 ** t)
        nhat = nu / (1 - cfg.b2 ** t)
        new["params"][k] = P[k] - lr * mhat / (torch.sqrt(nhat) + cfg.eps)
        new["mu"][k], new["nu"][k] = mu, nu
    aux["train_state_step"] = step
    aux["learning_rate"] = lr
    aux["grad_norm"] = float(gnorm)
    return new, aux


def forward_numpy(Pn, cfg, enc, action):
    """Independent numpy forward (no torch ops) used to cross-check ``forward``: the action logits."""
    B, T = action.shape
    E, hd = cfg.emb, cfg.emb // cfg.heads
    x = enc.reshape(B * T * cfg.enc_tokens, cfg.enc_dim).astype(np.float64)
    g = lambda k: np.asarray(Pn[k], np.float64)
    if cfg.use_adapter:
        a = np.maximum(x @ g("AdapterMLP_0/Dense_0/kernel") + g("AdapterMLP_0/Dense_0/bias"), 0)
        a = np.maximum(a @ g("AdapterMLP_0/Dense_1/kernel") + g("AdapterMLP_0/Dense_1/bias"), 0)
        res = 1 / (1 + np.exp(-g("residual_weight")))
        x = res * a + (1 - res) * x
    img = np.tanh(x.reshape(B, T, -1) @ g("image_text_input/kernel") + g("image_text_input/bias"))
    h = np.stack([img, g("action_input/embedding")[action]], 2).reshape(B, 2 * T, E)
    L = 2 * T

    def ln(z, s, b):
        mu = z.mean(-1, keepdims=True)
        return (z - mu) / np.sqrt(((z - mu) ** 2).mean(-1, keepdims=True) + 1e-6) * s + b

    for i in range(cfg.depth):
        p = f"policy/Block_{i}/"
        y = ln(h, g(p + "LayerNorm_0/scale"), g(p + "LayerNorm_0/bias"))
        qkv = y @ g(p + "Attention_0/Dense_0/kernel") + g(p + "Attention_0/Dense_0/bias")
        q, k, v = (t.reshape(B, L, cfg.heads, hd).transpose(0, 2, 1, 3) for t in np.split(qkv, 3, -1))
        s = q @ k.transpose(0, 1, 3, 2) * hd ** -0.5
        s = np.where(np.tril(np.ones((L, L), bool)), s, -np.inf)
        s = np.exp(s - s.max(-1, keepdims=True))
        s /= s.sum(-1, keepdims=True)
        y = (s @ v).transpose(0, 2, 1, 3).reshape(B, L, E)
        h = h + y @ g(p + "Attention_0/Dense_1/kernel") + g(p + "Attention_0/Dense_1/bias")
        y = ln(h, g(p + "LayerNorm_1/scale"), g(p + "LayerNorm_1/bias")) @ g(p + "FeedForward_0/fc1/kernel")
        y = 0.5 * y * (1 + np.tanh(np.sqrt(2 / np.pi) * (y + 0.044715 * y ** 3)))
        h = h + y @ g(p + "FeedForward_0/fc2/kernel")
    h = ln(h, g("policy/LayerNorm_0/scale"), g("policy/LayerNorm_0/bias"))
    n = "action_outputs_0"
    return np.maximum(h[:, 0::2] @ g(n + "/layers_0/kernel") + g(n + "/layers_0/bias"), 0) @ g(n + "/layers_2/kernel")
