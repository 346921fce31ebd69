"""CPU reference of the beam-search decode, in float64.

Built from the public functions of oracle/plank_oracle.py and following the cached loop of ``greedy_decode_cached``: the
decode runs B*K hypothesis rows (row b*K + k is beam k of drawing b) and after every step the batch dimension of every
per-row state (self-attention K / V caches, hidden-state cache, tokens, attach) is reordered by the new beams' parents.

Selection, as the HIP kernels implement it:
  * per row, the candidates are the vocab entries and the pointers j < t of ``last_row_dist`` (the self pointer j = t never),
    p = 0 never; the best K by p, ties to the smaller index; a pointer takes its token from the row's own history;
  * a finished row (one that has emitted END) has the single candidate (PAD, attach -1, log p 0);
  * per drawing, the K*K candidates ranked by score + log p descending, ties to the smaller parent beam, then the better rank;
  * at t = 0 only beam 0 of each drawing is live (the others start at -inf).
"""
from __future__ import annotations

import math

import torch

from oracle import plank_oracle as O


class _Stepper:
    """Cached decoder state of `rows` rows (greedy_decode_cached's loop body, one step per call)."""

    def __init__(self, p, cfg, batch, K, steps):
        d, H = cfg.d_model, cfg.n_head
        self.p, self.cfg, self.d, self.H, self.dh = p, cfg, d, H, d // H
        memory = O.encode(p, cfg, batch).repeat_interleave(K, dim=0)
        rows, S, _ = memory.shape
        self.rows = rows
        self.mem_mask = O.key_padding_additive(batch["input_mask"].repeat_interleave(K, dim=0)).to(memory.dtype)
        self.cross = []
        for i in range(cfg.n_dec):
            pre = f"decoder.layers.{i}.multihead_attn."
            w, b = p[pre + "in_proj_weight"], p[pre + "in_proj_bias"]
            k = O.linear(memory, w[d:2 * d], b[d:2 * d]).view(rows, S, H, self.dh).transpose(1, 2)
            v = O.linear(memory, w[2 * d:], b[2 * d:]).view(rows, S, H, self.dh).transpose(1, 2)
            self.cross.append((k, v))
        dt = memory.dtype
        self.self_k = [torch.zeros(rows, H, steps, self.dh, dtype=dt) for _ in range(cfg.n_dec)]
        self.self_v = [torch.zeros(rows, H, steps, self.dh, dtype=dt) for _ in range(cfg.n_dec)]
        self.hid = torch.zeros(rows, steps, d, dtype=dt)
        self.x_in = torch.zeros(rows, d, dtype=dt)

    def dist(self, t):
        """Run step t on x_in; returns last_row_dist [rows, V (+ t + 1)]."""
        p, cfg, d, H, dh, B = self.p, self.cfg, self.d, self.H, self.dh, self.rows
        scale = 1.0 / math.sqrt(dh)
        x = self.x_in
        for i in range(cfg.n_dec):
            pre = f"decoder.layers.{i}."
            w, b = p[pre + "self_attn.in_proj_weight"], p[pre + "self_attn.in_proj_bias"]
            qkv = O.linear(x, w, b)
            q = qkv[:, :d].view(B, H, 1, dh)
            self.self_k[i][:, :, t] = qkv[:, d:2 * d].view(B, H, dh)
            self.self_v[i][:, :, t] = qkv[:, 2 * d:].view(B, H, dh)
            s = (q @ self.self_k[i][:, :, :t + 1].transpose(-1, -2)) * scale
            o = (O.softmax_lastdim(s) @ self.self_v[i][:, :, :t + 1]).reshape(B, d)
            o = O.linear(o, p[pre + "self_attn.out_proj.weight"], p[pre + "self_attn.out_proj.bias"])
            x = O.layer_norm(x + o, p[pre + "norm1.weight"], p[pre + "norm1.bias"], cfg.eps_layer)
            w, b = p[pre + "multihead_attn.in_proj_weight"], p[pre + "multihead_attn.in_proj_bias"]
            q = O.linear(x, w[:d], b[:d]).view(B, H, 1, dh)
            ck, cv = self.cross[i]
            s = (q @ ck.transpose(-1, -2)) * scale + self.mem_mask
            o = (O.softmax_lastdim(s) @ cv).reshape(B, d)
            o = O.linear(o, p[pre + "multihead_attn.out_proj.weight"], p[pre + "multihead_attn.out_proj.bias"])
            x = O.layer_norm(x + o, p[pre + "norm2.weight"], p[pre + "norm2.bias"], cfg.eps_layer)
            hh = O.linear(x, p[pre + "linear1.weight"], p[pre + "linear1.bias"])
            hh = torch.relu(hh) if cfg.activation == "relu" else torch.nn.functional.gelu(hh)
            f = O.linear(hh, p[pre + "linear2.weight"], p[pre + "linear2.bias"])
            x = O.layer_norm(x + f, p[pre + "norm3.weight"], p[pre + "norm3.bias"], cfg.eps_layer)
        x = O.layer_norm(x, p["decoder.norm.weight"], p["decoder.norm.bias"], 1e-5)
        self.hid[:, t] = x
        return O.last_row_dist(p, cfg, self.hid[:, :t + 1])

    def reorder(self, idx):
        for i in range(self.cfg.n_dec):
            self.self_k[i] = self.self_k[i][idx]
            self.self_v[i] = self.self_v[i][idx]
        self.hid = self.hid[idx]

    def feed(self, tok, t):
        """next step's input: value[token] + coord[t % dof] + pos[t // dof] (models.py:120-132)"""
        p, cfg = self.p, self.cfg
        self.x_in = (p["input_embeddings.input_value.weight"][tok] + p["query_coord_embedding.weight"][t % cfg.out_dof]
                     + p["query_pos_embedding.weight"][t // cfg.out_dof])


def _params(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def beam_search(sd, cfg, batch, K, max_steps=None, early_stop=True, length_penalty=0.0, dtype=torch.float64, tie_tol=1e-5):
    """Returns a dict with ``beam_tokens`` / ``beam_attach`` [B, K, n], ``scores`` / ``finished`` / ``lengths`` [B, K] in
    final-ranking order (score / len^alpha, stable), ``tokens`` / ``attach`` [B, n] of the best beam, and ``near_tie``
    bool [B, steps]: at that step a ranking boundary the selection depends on was within ``tie_tol`` (the K-th and (K+1)-th
    merged scores absolute, or the K-th and (K+1)-th p of a live row relative)."""
    p = _params(sd, dtype)
    steps = int(max_steps or cfg.max_output_length)
    B = batch["input_value"].shape[0]
    R = B * K
    st = _Stepper(p, cfg, batch, K, steps)
    V, PAD, END = cfg.vocab, cfg.pad, cfg.end
    tokens = torch.zeros(R, steps, dtype=torch.long)
    attach = torch.full((R, steps), -1, dtype=torch.long)
    score = torch.full((R,), float("-inf"), dtype=dtype)
    score[::K] = 0.0
    fin = torch.zeros(R, dtype=torch.bool)
    fe = torch.full((R,), -1, dtype=torch.long)
    ties = []
    done = 0
    for t in range(steps):
        dist = st.dist(t)
        if dist.shape[1] > V:
            dist = dist[:, :V + t]                                   # the self pointer j = t is no candidate
        tie = torch.zeros(B, dtype=torch.bool)
        cands = []                                                   # per row: list of (log p, token, attach)
        for r in range(R):
            if bool(fin[r]):
                cands.append([(0.0, PAD, -1)])
                continue
            pr = dist[r]
            order = torch.sort(-pr, stable=True).indices             # p descending, ties to the smaller index
            top = order[:K + 1]
            lst = []
            for idx in top[:K].tolist():
                pv = float(pr[idx])
                if pv <= 0.0:
                    break
                if idx >= V:
                    lst.append((math.log(pv), int(tokens[r, idx - V]), idx - V))
                else:
                    lst.append((math.log(pv), idx, -1))
            cands.append(lst)
            if len(top) > K and math.isfinite(float(score[r])):
                a, b = float(pr[top[K - 1]]), float(pr[top[K]])
                if a > 0 and (a - b) <= tie_tol * a:
                    tie[r // K] = True
        parent = torch.empty(R, dtype=torch.long)
        new = []
        for b in range(B):
            pool = []
            for k in range(K):
                r = b * K + k
                for rank, (lp, tok, att) in enumerate(cands[r]):
                    pool.append((float(score[r]) + lp, k, rank, tok, att))
            pool.sort(key=lambda c: (-c[0], c[1], c[2]))
            if len(pool) > K and math.isfinite(pool[K - 1][0]) and pool[K - 1][0] - pool[K][0] <= tie_tol:
                tie[b] = True
            for k in range(K):
                s, kp, _, tok, att = pool[k]
                parent[b * K + k] = b * K + kp
                new.append((s, tok, att))
        ties.append(tie)
        tokens, attach = tokens[parent], attach[parent]
        fin, fe = fin[parent], fe[parent]
        st.reorder(parent)
        for r, (s, tok, att) in enumerate(new):
            score[r] = s
            tokens[r, t] = tok
            attach[r, t] = att
            if not bool(fin[r]) and tok == END:
                fin[r] = True
                fe[r] = t
        st.feed(tokens[:, t], t)
        done = t + 1
        if early_stop and bool(fin.all()):
            break
    n = int(fe.max()) + 1 if bool(fin.all()) else steps
    sc = score.view(B, K)
    lengths = torch.where(fe >= 0, fe + 1, torch.full_like(fe, steps)).view(B, K)
    key = sc / lengths.to(dtype) ** length_penalty if length_penalty != 0.0 else sc
    order = torch.sort(-key, dim=1, stable=True).indices
    bt = tokens.view(B, K, steps)[:, :, :n].gather(1, order[:, :, None].expand(B, K, n))
    ba = attach.view(B, K, steps)[:, :, :n].gather(1, order[:, :, None].expand(B, K, n))
    return {"tokens": bt[:, 0], "attach": ba[:, 0], "beam_tokens": bt, "beam_attach": ba, "scores": sc.gather(1, order),
            "finished": fin.view(B, K).gather(1, order), "lengths": lengths.gather(1, order),
            "near_tie": torch.stack(ties, dim=1), "steps": done}


def teacher_forced_logprob(sd, cfg, batch, beam_tokens, beam_attach, dtype=torch.float64):
    """Sum of log last_row_dist along given beams [B, K, n] (up to and including each beam's first END): what the beam's score
    must be.  The chosen entry of step t is V + attach when attach >= 0, else the token."""
    p = _params(sd, dtype)
    B, K, n = beam_tokens.shape
    R = B * K
    st = _Stepper(p, cfg, batch, K, n)
    tok = beam_tokens.reshape(R, n)
    att = beam_attach.reshape(R, n)
    total = torch.zeros(R, dtype=dtype)
    live = torch.ones(R, dtype=torch.bool)
    for t in range(n):
        dist = st.dist(t)
        idx = torch.where(att[:, t] >= 0, cfg.vocab + att[:, t], tok[:, t])
        pv = dist.gather(1, idx.clamp(max=dist.shape[1] - 1)[:, None])[:, 0]
        total = total + torch.where(live, torch.log(pv), torch.zeros_like(pv))
        live = live & (tok[:, t] != cfg.end)
        st.feed(tok[:, t], t)
    return total.view(B, K)
