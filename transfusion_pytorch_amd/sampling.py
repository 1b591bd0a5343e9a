"""KV-cached batched decoding: the reference's `sample_many` state machine (T:2082-2583) over the native engine.

Host bookkeeping follows the reference line by line; every tensor operation of a decoding step runs in the HIP kernels through a *decode plan*
(engine.Plan with a KV cache):

  * text step (T:2279-2349)     one new token per active sample: embed -> transformer against the cache -> fp32 logits
  * modality step (T:2354-2556) fixed-grid ODE (ode.py; torchdiffeq semantics) over the samples in the modality phase; every
    evaluation = latent_to_model -> transformer (FiLM path, t = step time) -> model_to_latent, against the conditional cache and - classifier-free
    guidance - the null-text cache: ONE forward over 2 B rows (the two caches are halves of one buffer)

One per-sample state machine (`_State`: phases text / modality / done; its methods and `Sampler._maybe_transition` are the only code that moves a
sample's phase, its parts and its cache / position / length counters) under two schedules.  Schedule: `_loop_continuous` while a mixed step stays
launch-bound (<= 4096 rows) - every global step advances every live sample by a token or by one ODE evaluation in one mixed forward: `step_roles` (what each guidance half of each sample brings) ->
`dense_layout` | `compact_layout` and the plan (`_step_plan`) -> `_load` -> `_mixed_step` (conditioning tables once per plan, row maps + solver
control of `ode.ode_control`, ode_stage, forward, ode_update) -> sample the text rows -> `_advance`; the null-text cache is prefilled once
(`_uncond_prefill`) and stays in lock-step.  Else `_loop_phased`, the reference's loop: `_text_rounds` until no sample is in its text phase, then
`_joint_ode` (`_ode_solve`), the null-text cache appended between phases (`_uncond_append`), not rebuilt.  `TFX_SAMPLE_SCHEDULE=continuous | phased`
forces one.  Roles and layouts are pure numpy over a host mirror of the states (tests/test_sampling_host_cpu.py).

Cache semantics reproduced exactly: the new [som] token is NOT in the conditional cache when its modality is decoded (the modality block takes
the rotary position the [som] would have had, T:2411); the K/V committed for a decoded modality are those of the LAST conditional ODE evaluation
(T:2531-2533); past modalities are conditioned at t = 1.
"""
from __future__ import annotations

import ctypes
import math
import os
from collections import namedtuple
from dataclasses import dataclass

import numpy as np
import torch

from . import capi
from .engine import Plan
from .ode import HIST_SLOTS, MULTISTEP, ode_control, ode_schedule


def _flat_len(parts):
    """cache rows a history takes"""
    return sum(math.prod(p[1].shape[:-1]) if isinstance(p, tuple) else len(p) for p in parts)


def _n_positions(parts):
    """rotary positions a history takes: a modality block takes one (T:398-415)"""
    return sum(1 if isinstance(p, tuple) else len(p) for p in parts)


@dataclass(slots=True)
class _State:                                   # _SamplingState, T:1270-1287 (token values mirrored on the host)
    parts: list                                 # host view of `sample`: lists of ints (text) and (type, tensor) tuples
    curr_seq: list                              # the text part currently being built (alias of parts[-1])
    last_token: int | None
    phase: str = 'text'
    cache_len: int = 0
    uncond_len: int = 0
    uncond_parts: int = 0                       # parts of `parts` whose tokens are in the null-text cache (incremental update between modality phases)
    uncond_pos: int = 0                         # rotary position the next token of the null-text history takes
    tokens_seen: int = 0
    num_past_modalities: int = 0
    curr_modality_id: int | None = None
    modality_shape: tuple | None = None
    modality_length: int | None = None
    num_tokens: int = 0
    forced: tuple = (None, None)
    unfed: bool = False                         # the last token of curr_seq was sampled but has not gone through the model yet
    ode_k: int = 0                              # continuous schedule: index of the next ODE evaluation of the modality being decoded
    som_pending: bool = False                   # continuous schedule: the null-text cache still lacks the [som] that opened the current modality
    commit_pending: bool = False                # continuous schedule: the null-text cache still lacks the modality just decoded (at t = 1)

    # Transitions.  `lockstep`: the null-text cache advances inside the same forwards as the conditional one (continuous schedule under guidance);
    # the phased schedule brings it up to date between phases instead (`_uncond_append`) and passes False.
    def budget(self, max_length):
        """the prefill's check of a sample that starts inside a modality"""
        if self.num_tokens > max_length:
            self.phase = 'done'

    def accept(self, tok, eos_id, max_length):
        """a sampled text token joins the sequence (T:2330-2349).  False: it ended the sample; True: the caller looks for a [som] (`_maybe_transition`)"""
        self.curr_seq.append(tok); self.last_token = tok; self.num_tokens += 1; self.unfed = True
        if tok == eos_id or self.num_tokens > max_length:
            self.phase = 'done'
            return False
        return True

    def fed(self, lockstep):
        """the token that was fed is in the caches - under `lockstep` its null id too, behind the block just committed where one was pending"""
        self.cache_len += 1; self.tokens_seen += 1; self.unfed = False
        if lockstep:
            if self.commit_pending:
                self.uncond_len += self.modality_length; self.uncond_pos += 1; self.commit_pending = False
            self.uncond_len += 1; self.uncond_pos += 1

    def begin_block(self, lockstep):
        """the first evaluation of a new block is next; a [som] that was sampled (not prompted) is still missing from the null-text cache"""
        self.ode_k, self.som_pending = 0, bool(lockstep and self.unfed)

    def som_fed(self):
        """the pending [som] is in the null-text cache (the conditional cache never takes it, T:2411)"""
        self.uncond_len += 1; self.uncond_pos += 1; self.som_pending = False

    def commit(self, block, eom_id, max_length, lockstep):
        """a decoded block joins the history with its [eom] as the next token to feed (T:2531-2556); its K/V are in the conditional cache already"""
        L = self.modality_length
        self.cache_len += L
        self.parts.append(block)
        self.curr_seq = [eom_id]; self.parts.append(self.curr_seq); self.last_token = eom_id; self.unfed = True
        self.tokens_seen += 1; self.num_tokens += L; self.num_past_modalities += 1
        self.phase = 'done' if self.num_tokens > max_length else 'text'
        self.commit_pending = bool(lockstep and self.phase == 'text')

    def null_prefilled(self, hist):
        """the null-text cache holds exactly the history `hist`"""
        self.uncond_len, self.uncond_parts, self.uncond_pos = _flat_len(hist), len(self.parts), _n_positions(hist)

    def null_appended(self, rows, pos):
        """everything in `parts` is in the null-text cache: `rows` more cache rows, the next rotary position is `pos` (`_uncond_append`)"""
        self.uncond_len, self.uncond_parts, self.uncond_pos = self.uncond_len + rows, len(self.parts), pos


@dataclass(frozen=True)
class _Call:                                    # the constants of one `sample_many` call
    B: int; H: int; use_cfg: bool; stream: int  # H: guidance halves of a forward - 2 under classifier-free guidance (`use_cfg`), else 1
    max_length: int; temperature: float; min_p: float; fixed_shape: tuple | None; init_noise: torch.Tensor | None
    modality_steps: int; cfg_scale: float       # modality_steps: grid points of the solver
    top_k: int | None = None; top_p: float | None = None     # text filters of tfx_sample_tokens_filtered (None = off)


def _filters_on(top_k, top_p):
    """whether a (validated) top-k / top-p pair filters at all: None, top_k 0 and top_p >= 1 are off"""
    return bool(top_k) or (top_p is not None and top_p < 1.)


def _draw(logits, V, V_draw, temperature, min_p, top_k, top_p, stream):
    """one sampler launch over the rows of a 2-d fp32 logits tensor: the launch of old (`tfx_sample_tokens`; `tfx_sample_tokens_range` when a draw
    range `V_draw` is given) with both filters off, `tfx_sample_tokens_filtered` otherwise.  One `torch.rand(B)` per call at a temperature
    either way, so a seeded run consumes the generator identically with and without filters.  Returns int32 ids on the device."""
    assert logits.dim() == 2 and logits.dtype == torch.float32 and logits.stride(1) == 1
    B = logits.shape[0]
    out = torch.empty(B, dtype=torch.int32, device=logits.device)
    u = torch.rand(B, device=logits.device) if temperature != 0. else None
    L, s = capi.lib(), ctypes.c_void_p(stream)
    if _filters_on(top_k, top_p):
        capi.check(L.tfx_sample_tokens_filtered(logits.data_ptr(), logits.stride(0), B, V, V if V_draw is None else V_draw, float(temperature),
                                                float(min_p), int(top_k or 0), 1. if top_p is None else float(top_p), capi.ptr(u), None, out.data_ptr(), s),
                   'tfx_sample_tokens_filtered')
    elif V_draw is None:
        capi.check(L.tfx_sample_tokens(logits.data_ptr(), logits.stride(0), B, V, float(temperature), float(min_p), capi.ptr(u), None, out.data_ptr(), s),
                   'tfx_sample_tokens')
    else:
        capi.check(L.tfx_sample_tokens_range(logits.data_ptr(), logits.stride(0), B, V, V_draw, float(temperature), float(min_p), capi.ptr(u), None,
                                             out.data_ptr(), s), 'tfx_sample_tokens_range')
    return out


def _sample_text_token(logits, V, temperature, min_p, stream, top_k=None, top_p=None):
    """sample_text_token (T:597-605) incl. min_p_filter (T:591-595) on the device, over the rows of a 2-d fp32 logits tensor (V valid columns);
    `top_k` / `top_p`: the filters of `tfx_sample_tokens_filtered` (include/tfx.h; not the reference's).  Returns int32 ids on the device."""
    return _draw(logits, V, None, temperature, min_p, top_k, top_p, stream)


def _pick_text_only(logits, V, N, temperature, min_p, stream, top_k=None, top_p=None):
    """the draw of `generate_text_only` (T:2690-2698) on the device: temperature 0 -> argmax over ALL V logits; else the min-p filter over all V
    logits (threshold relative to the global maximum), then the text-only mask (first N columns), then the draw.  `top_k` / `top_p` count and
    weigh the text tokens only (the candidates of `tfx_sample_tokens_filtered` are the draw range): the mask comes before them."""
    return _draw(logits, V, N if temperature != 0. else V, temperature, min_p, top_k, top_p, stream).long()


def _ode_axpy(y, f_cond, f_uncond, cfg_scale, a, stream):
    """out = y + a * (f_uncond + cfg_scale * (f_cond - f_uncond)) (or y + a * f_cond): one fused launch (tfx_ode_axpy)"""
    out = torch.empty_like(y)
    capi.check(capi.lib().tfx_ode_axpy(y.data_ptr(), f_cond.data_ptr(), capi.ptr(f_uncond), float(cfg_scale), float(a), out.data_ptr(), y.numel(),
                                       ctypes.c_void_p(stream)), 'tfx_ode_axpy')
    return out


def _ode_rk_axpy(y, K, ev, f_cond, f_uncond, cfg_scale, stream):
    """one evaluation of a Runge-Kutta step in dense form (tfx_ode_rk_axpy, one launch): the guided derivative goes to K[ev.q] unless the step ends
    here, and y + sum_{j<q} ev.w[j] K[j] + ev.w[q] g - the next stage's input, or the new state - is returned.  K: fp32 [3, *y.shape]"""
    out = torch.empty_like(y)
    w = tuple(ev.w) + (0.,) * (4 - len(ev.w))
    capi.check(capi.lib().tfx_ode_rk_axpy(y.data_ptr(), K.data_ptr(), y.numel(), ev.q, *w, f_cond.data_ptr(), capi.ptr(f_uncond), float(cfg_scale),
                                          None if ev.last else K[ev.q].data_ptr(), out.data_ptr(), y.numel(), ctypes.c_void_p(stream)), 'tfx_ode_rk_axpy')
    return out


def _ode_rk_solve(method, modality_steps, y, velocity, cfg_scale, stream):
    """the general stage loop of the dense sampling paths: `velocity(t, x)` -> (f_cond, f_uncond | None), contiguous fp32 of y's shape"""
    y = y.contiguous()
    K = torch.empty(3, *y.shape, device=y.device, dtype=torch.float32)
    x = y
    for ev in ode_schedule(method, modality_steps):
        fc, fu = velocity(ev.t, x)
        x = _ode_rk_axpy(y, K, ev, fc, fu, cfg_scale, stream)
        if ev.last:
            y = x
    return y


def _ode_ab_axpy(y, Hist, ev, f_cond, f_uncond, cfg_scale, stream):
    """one multistep step in dense form (tfx_ode_ab_axpy, one launch): y + sum_j ev.hw[j] Hist[ev.hr[j]] + ev.w[0] g is returned, the guided derivative
    g goes to Hist[ev.store] (a slot the same launch may read) unless no later step reads it.  Hist: fp32 [3, *y.shape]"""
    out = torch.empty_like(y)
    pad = HIST_SLOTS - len(ev.hr)
    capi.check(capi.lib().tfx_ode_ab_axpy(y.data_ptr(), *(Hist[s].data_ptr() for s in ev.hr), *(None,) * pad, *ev.hw, *(0.,) * pad, ev.w[0], f_cond.data_ptr(),
                                          capi.ptr(f_uncond), float(cfg_scale), Hist[ev.store].data_ptr() if ev.store >= 0 else None, out.data_ptr(),
                                          y.numel(), ctypes.c_void_p(stream)), 'tfx_ode_ab_axpy')
    return out


def _ode_ab_solve(method, modality_steps, y, velocity, cfg_scale, stream):
    """the dense loop of the Adams-Bashforth rules: the start-up steps are `_ode_rk_solve`'s launches (their stage-0 derivative copied from K[0] to its
    history slot on the device), every later step is one evaluation and one tfx_ode_ab_axpy"""
    y = y.contiguous()
    K, Hist = (torch.empty(3, *y.shape, device=y.device, dtype=torch.float32) for _ in range(2))
    x = y
    for ev in ode_schedule(method, modality_steps):
        fc, fu = velocity(ev.t, x)
        if ev.hr:
            x = _ode_ab_axpy(y, Hist, ev, fc, fu, cfg_scale, stream)
        else:
            x = _ode_rk_axpy(y, K, ev, fc, fu, cfg_scale, stream)
            if ev.store >= 0:
                Hist[ev.store].copy_(K[0])
        if ev.last:
            y = x
    return y


def _ode_solve(method, modality_steps, y, velocity, cfg_scale, stream):
    """one solve of the dense sampling paths over the grid linspace(0, 1, modality_steps), `velocity` as in `_ode_rk_solve`.  The midpoint rule keeps
    its own kernel: y_mid = y + dt / 2 f(t0, y), y <- y + dt f(t0 + dt / 2, y_mid), one tfx_ode_axpy each; the multistep rules are `_ode_ab_solve`,
    every other rule is `_ode_rk_solve`."""
    if method in MULTISTEP:
        return _ode_ab_solve(method, modality_steps, y, velocity, cfg_scale, stream)
    if method != 'midpoint':
        return _ode_rk_solve(method, modality_steps, y, velocity, cfg_scale, stream)
    x = y = y.contiguous()
    for ev in ode_schedule(method, modality_steps):
        fc, fu = velocity(ev.t, x)
        x = _ode_axpy(y, fc, fu, cfg_scale, ev.w[ev.q], stream)
        if ev.last:
            y = x
    return y


# ---------------------------------------------------------------------- one step of the continuous schedule, on the host (pure numpy)
# host mirror of the per-sample state, an [11, B] int64 array with one column per sample (the step's index arrays are built from it with array operations):
# phase (0 done / 1 text / 2 modality), cache_len, uncond_len, tokens_seen, uncond_pos, last_token, modality length, type, ode_k, som_pending, commit_pending
PH, CL, UL, TS, UP, LT, LL, TY, OK, SP, CP = range(11)
_PHASE_CODE = {'done': 0, 'text': 1, 'modality': 2}

# What every unit (guidance half h, sample i) = cache row h B + i brings to a step.  [B]: is_t / is_m (phase), com (null-text half: the block just
# decoded goes in, prompt-style at t = 1, ahead of the next token), L, ty, k (ode_k).  [H, B]: base (keys already cached);
#   blk  it carries a block of L rows: cache offset boff, rotary position rblk, instance iblk = index of its conditioning time (n_t - 1: t = 1)
#   txt  it carries one token row: id itxt, cache offset tbase, rotary position trot
Roles = namedtuple('Roles', 'is_t is_m com L ty k base blk boff rblk iblk txt itxt tbase trot')


def step_roles(A, H, n_t, null_id):
    B = A.shape[1]
    is_t, is_m = A[PH] == 1, A[PH] == 2
    com = is_t & (A[CP] > 0)
    def halves(cond, null):                                     # [H, B]: row 0 the real history's, row 1 the null-text history's
        out = np.empty((H, B), cond.dtype)
        out[0], out[1:] = cond, null
        return out
    none = np.zeros(B, bool)
    base = halves(A[CL], A[UL])
    txt_first = halves(none, is_m & (A[SP] > 0))                # null-text half: the [som] the real history never feeds (T:2411), ahead of the block
    blk_first = halves(none, com)
    both = lambda a: np.broadcast_to(a, (H, B))
    return Roles(is_t, is_m, com, A[LL], A[TY], A[OK], base,
                 blk=is_m | blk_first, boff=base + txt_first,
                 rblk=both(np.where(is_m, A[TS], A[UP])),       # an ODE block sits at tokens_seen in BOTH halves; a finished one at its history position
                 iblk=both(np.where(is_m, A[OK], n_t - 1)),
                 txt=is_t | txt_first, itxt=halves(A[LT], null_id),
                 tbase=base + np.where(blk_first, A[LL], 0),
                 trot=np.where(is_t, halves(A[TS], A[UP] + com), A[UP]))


# A step's rows in one of the two layouts: the five index arrays `_load` takes, `units` (compacted plans: the 4 U per-unit arrays of Plan `units`), and -
# the common form the rest of a mixed step reads - blk_rows (which rows are block rows), row_ty (each row's modality type), unit_row0 (each unit's first row)
Layout = namedtuple('Layout', 'ids pos kve rot tok_inst units blk_rows row_ty unit_row0')


def dense_layout(r, Lq, cap):
    """Lq rows for EVERY unit, done or not: a block in columns 0 .. L - 1, the token in column Lq - 1; arrays of shape [H, B, Lq]"""
    H, B = r.base.shape
    jj = np.arange(Lq, dtype=np.int64)
    unit = np.arange(H * B, dtype=np.int64).reshape(H, B)
    col = lambda a: a[:, :, None]
    has_blk = col(r.blk) & (jj < r.L[:, None])
    ids = np.zeros((H, B, Lq), np.int32)
    pos = np.where(has_blk, col(unit * cap + r.boff) + jj, -1)
    kve = np.where(has_blk, col(r.boff + r.L), col(np.maximum(r.base, 1)))
    rot = np.where(has_blk, col(r.rblk), 0)
    tok_inst = np.where(has_blk, col(r.iblk), -1)
    ids[:, :, -1] = np.where(r.txt, r.itxt, 0)
    pos[:, :, -1] = np.where(r.txt, unit * cap + r.tbase, pos[:, :, -1])
    kve[:, :, -1] = np.where(r.txt, r.tbase + 1, kve[:, :, -1])
    rot[:, :, -1] = np.where(r.txt, r.trot, rot[:, :, -1])
    row_ty = np.broadcast_to(r.ty[None, :, None], (H, B, Lq)).reshape(-1)
    return Layout(ids, pos, kve, rot, tok_inst, None, has_blk.reshape(-1), row_ty, unit.reshape(-1) * Lq)


def compact_layout(r, step, cap):
    """exactly the rows the live units need - a block's L rows, then the token row - packed back to back, unit u owning rows unit_row0[u] .. + cnt[u] of
    the plan (Plan `units`; the attention kernel reads its query rows through them, tfx_attn_args.q_row0 / q_cnt).  The dense layout spends L + 1 rows
    on every sample: 640 rows per step at config 5 against ~270 needed.  Arrays of length Tb, the row count rounded up to the bucket `step`."""
    H, B = r.base.shape
    U = H * B
    Lu = np.broadcast_to(r.L, (H, B)).reshape(-1)
    nblk = np.where(r.blk.reshape(-1), Lu, 0)
    cnt = nblk + r.txt.reshape(-1)
    row0 = np.cumsum(cnt) - cnt
    Ts = int(cnt.sum())
    Tb = max(step, -(-Ts // step) * step)
    u = np.repeat(np.arange(U, dtype=np.int64), cnt)
    j = np.arange(Ts, dtype=np.int64) - row0[u]
    isb = j < nblk[u]
    f = lambda a: a.reshape(-1)[u]
    ids = np.zeros(Tb, np.int32); pos = np.full(Tb, -1, np.int64); kve = np.ones(Tb, np.int64); rot = np.zeros(Tb, np.int64); tok_inst = np.full(Tb, -1, np.int64)
    ids[:Ts] = np.where(isb, 0, f(r.itxt))
    pos[:Ts] = u * cap + np.where(isb, f(r.boff) + j, f(r.tbase))
    kve[:Ts] = np.where(isb, f(r.boff) + Lu[u], f(r.tbase) + 1)
    rot[:Ts] = np.where(isb, f(r.rblk), f(r.trot))
    tok_inst[:Ts] = np.where(isb, f(r.iblk), -1)
    blk_rows = np.zeros(Tb, bool); blk_rows[:Ts] = isb
    row_ty = np.zeros(Tb, np.int64); row_ty[:Ts] = np.broadcast_to(r.ty, (H, B)).reshape(-1)[u]
    units = np.zeros(4 * U, np.int32)
    units[:U] = row0; units[U:2 * U] = cnt
    units[2 * U:3 * U] = np.where(r.blk.reshape(-1), row0, -1)
    units[3 * U:3 * U + B] = np.where(r.txt[0], row0[:B] + nblk[:B], 0)
    return Layout(ids, pos, kve, rot, tok_inst, units, blk_rows, row_ty, row0)


# continuous schedule: compacted mixed steps (1) instead of the dense (L + 1)-rows-per-sample layout.  Built, token-identical (tests/test_sampling_gpu.py runs
# both) - and OFF by default: config 5 measured 1.630 s against 1.646 s (same box).  A decode step's time is flat in its row count between ~256 and 640 rows
# (tools/bench_decode_step.py: 2.9 - 3.3 ms for 128 samples x 2 / 3 / 5 rows, 2.3 ms at 128 x 1): it is ~225 dependent launches of 6 - 20 us each, set by
# launch ramps and first-load latencies, not by rows - the rows were never what a step paid for.
_COMPACT = os.environ.get('TFX_DECODE_COMPACT', '0') == '1'
_COMPACT_STEP = int(os.environ.get('TFX_DECODE_COMPACT_STEP', '128'))     # row-count bucket of the compacted plans (a plan = buffers + launch list + hipGraph per bucket)


class _Blocks:
    """continuous schedule: the blocks being decoded.  Y [B][Lc][dmax] is the ODE state of every sample, Ym the midpoint state or (tableau rules) K, the stage
    derivatives [3][B][Lc][dmax], Hist (multistep rules) the history ring [3][B][Lc][dmax]; `sel` [M][B] says per type which samples decode a block of that
    type; A is the host mirror of the sample states."""

    def __init__(self, smp, c, ctl, cond_times):
        self.smp, self.c, self.ctl, self.cond_times = smp, c, ctl, cond_times     # ctl: ode.ode_control; cond_times: its times + [1.] on the device
        self.rk = smp.m.ode_method != 'midpoint'                                  # the tableau rules: tfx_ode_rk_stage / tfx_ode_rk_update
        self.ab = smp.m.ode_method in MULTISTEP                                   # tfx_ode_rk_stage / tfx_ode_ab_update
        self.Lc, self.Y, self.Ym, self.Hist = 0, None, None, None
        M = smp.m.num_modalities
        self.sel = torch.zeros(M, c.B, device=smp.dev) if M > 1 else None
        self.A = np.zeros((11, c.B), np.int64)

    def begin(self, i, st):
        """sample i starts a block: room for its rows, its initial noise, evaluation 0 next"""
        smp, B = self.smp, self.c.B
        L, dmax = st.modality_length, max(smp.md.dim_latents)
        if L > self.Lc:
            newY, newYm = torch.zeros(B, L, dmax, device=smp.dev), torch.zeros(*((3,) if self.rk else ()), B, L, dmax, device=smp.dev)
            newHist = torch.zeros(HIST_SLOTS, B, L, dmax, device=smp.dev) if self.ab else None
            if self.Y is not None:
                newY[:, :self.Lc], newYm[..., :self.Lc, :] = self.Y, self.Ym
                if self.ab:
                    newHist[:, :, :self.Lc] = self.Hist
            self.Y, self.Ym, self.Hist, self.Lc = newY, newYm, newHist, L
        smp._init_noise(self.Y[i], st, self.c)
        st.begin_block(self.c.use_cfg)
        if self.sel is not None:
            self.sel[:, i] = 0.; self.sel[st.curr_modality_id, i] = 1.

    def mirror(self, states, which):
        """the columns `which` of A from their states (one array assignment: a column at a time costs more than the transitions themselves)"""
        cols = [(_PHASE_CODE[st.phase], st.cache_len, st.uncond_len, st.tokens_seen, st.uncond_pos, st.last_token if st.last_token is not None else 0,
                 st.modality_length or 0, st.curr_modality_id or 0, st.ode_k, st.som_pending, st.commit_pending) for st in map(states.__getitem__, which)]
        self.A[:, which] = np.array(cols, np.int64).reshape(-1, 11).T


class Sampler:
    def __init__(self, model):
        self.m = model
        self.dev = model.device
        self.md = model.md
        self.pos_emb_in_decode = False                                # `sample_many` sets it: the blocks being decoded carry their axial positional embedding
        self._grew = False                                            # the call had to grow its KV cache (and so rebuilt its plans)
        self._stage = {}                                              # rings of pinned staging buffers (`_pinned`)

    # ------------------------------------------------------------------ prompt handling (T:1701-1800)
    def _meta_tokens(self, shape, ty):
        m = self.m
        s = ','.join(map(str, shape))
        return [m.meta_id] + [ord(c) + m.meta_id + 1 for c in s] + [m.som_ids[ty]]

    def _prepare(self, prompt, force_modality_at_start):
        m = self.m
        if torch.is_tensor(prompt) and prompt.is_floating_point():
            prompt = (0, prompt)
        if torch.is_tensor(prompt):                                   # text only prompt
            prompt = [prompt]
        elif isinstance(prompt, tuple):
            ty, mod = prompt
            shape = tuple(mod.shape[:-1])
            prompt = [self._meta_tokens(shape, ty), (ty, mod), [m.eom_ids[ty]]]
        elif prompt is None:
            prompt = []
        prompt = [p for p in prompt if p is not None]
        if prompt and isinstance(prompt[-1], tuple):                  # a raw modality ending the prompt is closed with its [eom]
            prompt.append([m.eom_ids[prompt[-1][0]]])
        parts = [[m.sos_id]]
        for p in prompt:
            if isinstance(p, tuple):
                parts.append((p[0], p[1].to(self.dev, torch.float32)))
                continue
            ids = p if isinstance(p, list) else [int(v) for v in torch.atleast_1d(p).reshape(-1).tolist()]
            if isinstance(parts[-1], list):                           # concat_contiguous_text, T:204-222
                parts[-1] = parts[-1] + ids
            else:
                parts.append(list(ids))
        forced_id, forced_shape = force_modality_at_start if isinstance(force_modality_at_start, tuple) else (force_modality_at_start, None)
        if forced_id is not None:                                     # maybe_force_modality_at_start, T:1701-1731
            toks = self._meta_tokens(forced_shape, forced_id) if forced_shape is not None else [m.som_ids[forced_id]]
            if isinstance(parts[-1], list):
                parts[-1] = parts[-1] + toks
            else:
                parts.append(toks)
        return parts, forced_id, forced_shape

    def _shape_from_seq(self, seq, ty, fixed_shape, forced_shape):    # get_modality_shape_from_seq, T:1607-1648
        m = self.m
        shape = forced_shape if forced_shape is not None else fixed_shape
        default_shape = m.modality_default_shape[ty]
        if m.meta_id in seq and forced_shape is None:
            after = seq[len(seq) - 1 - seq[::-1].index(m.meta_id) + 1:]
            meta = after[:-1]
            meta_str = ''.join(chr(min(max(t - (m.meta_id + 1), 0), 127)) for t in meta)
            if len(after) > 0:
                if not meta_str.isdigit() or int(meta_str) <= 0:
                    assert default_shape is not None, 'invalid modality meta information detected, please set `modality_default_shape` in order to properly fallback'
                    shape = default_shape
                else:
                    shape = m.to_modality_shape_fn[ty](meta_str)
        shape = shape if shape is not None else default_shape
        ndim = m.modality_num_dim[ty]
        if m.fallback_to_default_shape_if_invalid and ndim is not None and len(shape) != ndim:
            shape = default_shape
        assert shape is not None, f'language model did not produce a proper modality shape for modality type {ty} - please set a fallback shape with `modality_default_shape`'
        assert ndim is None or ndim == len(shape), f'expected modality type {ty} to have {ndim} dimensions but language model produced a shape of {shape}'
        return tuple(shape)

    def _maybe_transition(self, st, fixed_shape):                     # T:2203-2224 / get_modality_transition T:1802-1825
        m = self.m
        tok = st.curr_seq[-1]
        if tok not in m.som_ids:
            return False
        ty = m.som_ids.index(tok)
        forced_id, forced_shape = st.forced
        shape = self._shape_from_seq(st.curr_seq, ty, fixed_shape, forced_shape if ty == forced_id else None)
        st.curr_modality_id, st.modality_shape, st.modality_length, st.phase = ty, shape, math.prod(shape), 'modality'
        return True

    def _commit(self, st, y, c, lockstep):
        """the block just decoded - the sample's rows `y` of the ODE state - joins its history, T:2531-2556"""
        ty = st.curr_modality_id
        L, dl = st.modality_length, self.md.dim_latents[ty]
        st.commit((ty, y[:L, :dl].reshape(*st.modality_shape, dl).clone()), self.m.eom_ids[ty], c.max_length, lockstep)

    def _init_noise(self, y, st, c):
        """the initial noise of a new block into the sample's rows `y` of the ODE state"""
        L, dl = st.modality_length, self.md.dim_latents[st.curr_modality_id]
        y[:L, :dl] = c.init_noise[:L, :dl].to(self.dev) if c.init_noise is not None else torch.randn(L, dl, device=self.dev)

    def _as_batch(self, parts_list, null_text=False):
        """host parts -> the list-of-tensors batch format the packer takes."""
        out = []
        for parts in parts_list:
            s = []
            for p in parts:
                if isinstance(p, tuple):
                    s.append(p)
                else:
                    ids = [self.m.null_text_id] * len(p) if null_text else p
                    s.append(torch.tensor(ids, dtype=torch.long, device=self.dev))
            out.append(s)
        return out

    def _initial_states(self, prompts, force_modality_at_start):
        if prompts is None:
            prompts = [None]
        elif not isinstance(prompts, list):
            prompts = [prompts]
        states = []
        for prompt in prompts:
            parts, forced_id, forced_shape = self._prepare(prompt, force_modality_at_start)
            last = parts[-1]                                          # always text: `_prepare` closes a trailing modality with its [eom]
            states.append(_State(parts=parts, curr_seq=last, last_token=last[-1], forced=(forced_id, forced_shape), cache_len=_flat_len(parts),
                                 tokens_seen=_n_positions(parts), num_past_modalities=sum(isinstance(p, tuple) for p in parts)))
        return states

    # ------------------------------------------------------------------ caches
    def _alloc_cache(self, B, maxlen):
        return torch.zeros(self.md.depth, B, maxlen, 2 * self.md.hdk, device=self.dev, dtype=torch.bfloat16)

    def _fill_cache(self, cache, plan, B, n):
        D, hd, ldq = self.md.depth, self.md.hdk, self.md.ldq
        cache[:, :, :n, :hd].copy_(plan.qkr.view(D, B, n, 2 * hd)[..., hd:])
        cache[:, :, :n, hd:].copy_(plan.qkvg.view(D, B, n, ldq)[..., 2 * hd:3 * hd])

    def _decode_plan(self, key, B, Lq, cache, with_latents, n_inst=None, tile_attn=False, units=None, ctl_rows=2):
        plans = self.m._decode_plans
        if key not in plans:
            R = {t: B * Lq for t in range(self.m.num_modalities)} if with_latents else {}
            self.m.store.refresh_shadows(self.m._stream())
            p = Plan(self.m.store, B, Lq, (n_inst or B) if with_latents else 0, R, training=False, cache=cache, tile_attn=tile_attn, units=units, ctl_rows=ctl_rows)
            p.q_start.zero_()
            plans[key] = p
        return plans[key]

    def _kept_cache(self, rows, need, keep_key):
        """Decode plans - launch lists, their captured graphs, per-plan AdaLN tables of the solver's time grid - are bound to the cache buffer they were
        built on.  A serving process calls sample_many over and over with the same geometry: the buffer and its plans are KEPT on the model between
        calls (plan build + graph capture were ~30 ms of every call) and reused while everything they froze (`keep_key`) still
        holds.  TFX_DECODE_KEEP=0 (keep_key None) turns it off; TFX_DECODE_KEEP_GB bounds the kept cache (default 16); `model.train()` drops it."""
        m = self.m
        ent = getattr(m, '_decode_keep', None) if keep_key is not None else None
        if ent is not None and ent['key'] == keep_key and ent['joint'].shape[2] >= need:
            joint, m._decode_plans = ent['joint'], ent['plans']
            joint.zero_()
        else:
            m._decode_keep = None
            m._decode_plans = {}
            joint = self._alloc_cache(rows, need)
        return joint

    def _keep_cache(self, joint, keep_key):
        m = self.m
        gib = joint.numel() * joint.element_size() / 2 ** 30
        if keep_key is not None and not self._grew and gib <= float(os.environ.get('TFX_DECODE_KEEP_GB', '16')):
            m._decode_keep = {'key': keep_key, 'joint': joint, 'plans': m._decode_plans}      # (a run that had to grow its cache rebuilt its plans: not kept)
        else:
            m._decode_keep = None
        m._decode_plans = {}

    # ------------------------------------------------------------------ main
    def sample_many(self, prompts, max_length, text_temperature, text_min_p, fixed_modality_shape, force_modality_at_start,
                    init_modality_noise, modality_steps, cfg_scale, pos_emb_in_decode=False, text_top_k=None, text_top_p=None):
        m, md, dev = self.m, self.md, self.dev
        self.pos_emb_in_decode, self._grew = pos_emb_in_decode, False
        m._require_gpu()
        states = self._initial_states(prompts, force_modality_at_start)
        B = len(states)
        # classifier-free guidance evaluates every ODE step twice - against the real history and against the null-text one (T:2468-2525).  Both
        # evaluations share the weights and a decode step is launch-bound, so they run as ONE forward over 2 B rows: the two KV caches are the halves
        # of one buffer (the text steps use the first half through a view)
        use_cfg = cfg_scale != 1.
        c = _Call(B, 2 if use_cfg else 1, use_cfg, m._stream(), max_length, text_temperature, text_min_p, fixed_modality_shape, init_modality_noise,
                  modality_steps, cfg_scale, text_top_k, text_top_p)

        # ---- batched prefill (T:2194-2201): prompted modalities conditioned at t = 1, no meta tokens re-added
        max_past = max((s.num_past_modalities for s in states), default=0)
        times = torch.ones(B, max(max_past, 1), device=dev)
        plan, S = m._forward_plain(self._as_batch([s.parts for s in states]), times, add_meta=False)
        n0 = S['n']
        est = [math.prod(sh) for sh in m.modality_default_shape if sh is not None]
        Lcap = max(est + [math.prod(fixed_modality_shape or (1,)), 16])
        maxlen = (max(s.cache_len for s in states) + max_length + 2 * Lcap + 80) // 64 * 64
        # what the kept plans froze: rows, solver and its grid, guidance on / off, the parameter version (shadows and cond tables are functions of the weights)
        keep_key = (c.H * B, int(modality_steps), bool(use_cfg), m.store.params_version(), tuple(fixed_modality_shape or ()), bool(pos_emb_in_decode), m.ode_method)
        if os.environ.get('TFX_DECODE_KEEP', '1') == '0':
            keep_key = None
        joint = self._kept_cache(c.H * B, max(maxlen, n0), keep_key)
        self._fill_cache(joint[:, :B], plan, B, n0)
        for st in states:
            self._maybe_transition(st, fixed_modality_shape)
        last_rows = torch.tensor([i * n0 + s.cache_len - 1 for i, s in enumerate(states)], device=dev)
        first = _sample_text_token(plan.logits.index_select(0, last_rows), md.vocab, text_temperature, text_min_p, c.stream, c.top_k, c.top_p).tolist()
        for st, tok in zip(states, first):
            if st.phase != 'text':
                st.budget(max_length)
            elif st.accept(tok, m.eos_id, max_length):
                self._maybe_transition(st, fixed_modality_shape)

        # Two schedules over the same per-sample state machine (samples only ever attend to their own cache, so the schedule cannot change
        # what a sample decodes - the reference's own test asserts sample_many == per-prompt sample_one).  A mixed step of the continuous one carries
        # (modality length + 1) rows for EVERY sample, a text step of the phased loop one: continuous batching pays while a forward is launch-bound
        # (its time does not depend on the row count) - up to a few thousand rows.  Long blocks (images) in a large batch keep the phased schedule:
        # there a mixed step would cost as much as a joint ODE evaluation of the whole batch.
        schedule = os.environ.get('TFX_SAMPLE_SCHEDULE', 'auto')
        if schedule == 'auto':
            est = est + ([math.prod(fixed_modality_shape)] if fixed_modality_shape else [])
            schedule = 'continuous' if c.H * B * (max(est, default=4) + 1) <= 4096 else 'phased'
        (self._loop_phased if schedule == 'phased' else self._loop_continuous)(states, joint, c)
        self._keep_cache(joint, keep_key)
        return [[(p if isinstance(p, tuple) else torch.tensor(p, dtype=torch.long, device=dev)) for p in st.parts] for st in states]

    def _pinned(self, name, shape, dtype, zero=False):
        """pinned host staging buffers, a ring of 8 per (name, shape): the per-step control arrays go up as asynchronous copies (a pinned allocation per
        step costs more than the step's copy; a text step ends in a host sync, a run of modality steps issues at most four uploads before one)"""
        ring = self._stage
        key = (name, tuple(shape), dtype)
        if key not in ring:
            ring[key] = [[(torch.zeros if zero else torch.empty)(shape, dtype=dtype, pin_memory=True) for _ in range(8)], 0]
        bufs, k = ring[key]
        ring[key][1] = (k + 1) % len(bufs)
        return bufs[k]

    def _uncond_prefill(self, joint, states, hist, who, room):
        """null-text twin of a prefill (T:2386-2406): the histories `hist`, one per sample - every text token as the null id, modalities at t = 1 - go
        through the model and their keys / values into the second half of the joint cache (grown to hold `room` rows more); the samples `who` then
        have exactly their `hist` in it.  Returns the joint cache."""
        m, B = self.m, len(states)
        past = max(max((states[i].num_past_modalities for i in who), default=0), 1)
        uplan, US = m._forward_plain(self._as_batch(hist, null_text=True), torch.ones(B, past, device=self.dev), add_meta=False)
        if joint.shape[2] < US['n'] + room:
            joint = self._grow(joint, US['n'] + room)
        self._fill_cache(joint[:, B:], uplan, B, US['n'])
        for i in who:
            states[i].null_prefilled(hist[i])
        return joint

    # ------------------------------------------------------------------ continuous schedule
    def _loop_continuous(self, states, joint, c):
        """Continuous batching of the decode loop.  The reference's schedule (and `_loop_phased`) makes the samples that reached a [som] wait until
        the slowest writer of the round has reached its own, then decodes all waiting modalities in one joint ODE: with B desynchronised samples the
        text phase runs sum over rounds of max_i(text run) steps.  Here every global step is ONE forward over (1 | 2) B x Lq rows in which each live
        sample advances by what it needs: a text sample feeds its last token (one row), a sample inside a modality runs its next ODE evaluation
        (L rows at its own step time - the fixed-grid solver as a per-sample state machine on the device), and the null-text half of
        classifier-free guidance stays in lock-step - the null id of the same token, the same evaluation against its own cache, and, right
        after a modality is finished, that block once more at t = 1 (what the reference's re-prefill of the null-text history computes, T:2386-2406).
        The run takes max_i(tokens_i + evaluations_i) steps instead.  Row roles and cache positions follow `_load_modality` / `_uncond_append`."""
        m, md, dev, B = self.m, self.md, self.dev, c.B
        ctl = ode_control(m.ode_method, c.modality_steps)
        # The time conditioning of a decode step - Fourier features -> MLP -> every layer's AdaLN tables, a GEMM that streams ALL the conditioning
        # weights (1.2 GB at dim 1024 / depth 24: 0.5 ms of a 4 ms step) - depends on the step time alone, and a fixed-grid solver only ever asks
        # for stages x (S - 1) times plus t = 1 (finished blocks).  The "instances" of the mixed plan are therefore those TIMES: their tables are computed
        # once per plan, a token's instance index says which row it reads, and the conditioning launches drop out of the per-step replay.
        cond_times = torch.tensor(ctl.times + (1.,), dtype=torch.float32, device=dev)
        n_t = cond_times.numel()
        if c.use_cfg:
            # null-text twin of the prefill: every token that went through the model so far (the sampled-but-unfed last token excluded)
            fed = [st.parts[:-1] + [st.parts[-1][:-1]] if st.unfed else st.parts for st in states]
            joint = self._uncond_prefill(joint, states, [[p for p in h if isinstance(p, tuple) or len(p)] for h in fed], range(B), 0)
        blocks = _Blocks(self, c, ctl, cond_times)
        A = blocks.A
        for i, st in enumerate(states):
            if st.phase == 'modality':
                blocks.begin(i, st)
        blocks.mirror(states, np.arange(B))
        async_steps = 0
        while A[PH].any():
            r = step_roles(A, c.H, n_t, m.null_text_id)
            mixed = bool(r.is_m.any() or r.com.any())
            Lq = blocks.Lc + 1 if mixed else 1
            need = int(max(A[CL].max(), A[UL].max())) + Lq + 2
            if need > joint.shape[2]:
                joint = self._grow(joint, need + 192)
            p, lay = self._step_plan(r, mixed, Lq, joint, n_t, 1 + len(ctl.rows))
            self._load(p, lay.ids.reshape(-1), lay.pos.reshape(-1), lay.kve.reshape(-1), lay.rot.reshape(-1), lay.tok_inst.reshape(-1), units=lay.units)
            if mixed:
                self._mixed_step(p, lay, r, Lq, blocks, states, c)
            else:
                self._run(p, c.stream, 0, p.fwd_logits_end)
            toks = None
            if r.is_t.any():
                lg = p.logits.view(c.H * B, Lq, md.vp)[:B, Lq - 1] if lay.units is None else p.logits.view(p.T, md.vp).index_select(0, p.unit_txt[:B])
                toks = _sample_text_token(lg, md.vocab, c.temperature, c.min_p, c.stream, c.top_k, c.top_p).tolist()      # host sync
                async_steps = 0
            else:
                async_steps += 1
                if async_steps >= 4:                                        # the staging rings are 8 deep: never run further ahead of the device
                    torch.cuda.current_stream(dev).synchronize(); async_steps = 0
            self._advance(states, toks, blocks, len(ctl.times), c)

    def _step_plan(self, r, mixed, Lq, joint, n_t, ctl_rows):
        """the plan of a step and the step's rows in that plan's layout.  One attention kernel - the tiled forward kernel - for every plan of the run: a
        token's arithmetic must not depend on which plan carried it.  Compacted plans come in row-count buckets of `_COMPACT_STEP`."""
        nb, cap, method = r.base.size, joint.shape[2], self.m.ode_method
        if mixed and _COMPACT:
            lay = compact_layout(r, _COMPACT_STEP, cap)
            Tb = lay.ids.size
            p = self._decode_plan(('mixc', nb, Tb, Lq, joint.data_ptr(), method), Tb, 1, joint, True, n_inst=n_t, tile_attn=True, units=(nb, Lq), ctl_rows=ctl_rows)
        else:
            lay = dense_layout(r, Lq, cap)
            p = self._decode_plan(('mix' if mixed else 'txt', nb, Lq, joint.data_ptr(), method), nb, Lq, joint, mixed, n_inst=n_t, tile_attn=True, ctl_rows=ctl_rows)
        return p, lay

    def _mixed_step(self, p, lay, r, Lq, blocks, states, c):
        """a step with block rows: every sample inside a modality runs one evaluation of its solver - stage input from the ODE state (ode_stage), the
        forward, the state update from the predicted flow (ode_update) - next to the text rows and the finished blocks of the null-text half"""
        m, md, B, H, stream = self.m, self.md, c.B, c.H, c.stream
        M, dmax, sp = m.num_modalities, max(md.dim_latents), ctypes.c_void_p(c.stream)
        lib = capi.lib()
        ode_stage, ode_update = (lib.tfx_ode_rk_stage, lib.tfx_ode_ab_update if blocks.ab else lib.tfx_ode_rk_update) if blocks.rk else (lib.tfx_ode_stage, lib.tfx_ode_update)
        unit_blk0 = p.unit_blk0.data_ptr() if lay.units is not None else None
        Y, Ym, Lc = blocks.Y, blocks.Ym, blocks.Lc
        hist = (blocks.Hist.data_ptr(),) if blocks.ab else ()        # the multistep rules' ring, next to the stage derivatives
        if not getattr(p, '_cont_ready', False):
            for t in range(M):
                p.row_inst[t].zero_()
                p.set_noise(t, None)
            p.inst_time.copy_(blocks.cond_times)
            Plan.run(p.fwd, stream, *p.fwd_cond)                      # the AdaLN tables of every time the solver will ask for, once
            p._cont_ready = True
        self._upload_row_maps(p, lay, r, blocks.ctl)
        if md.model_output_clean:                                   # the clean-prediction conversion reads a row's time through its instance
            for t in range(M):
                p.row_inst[t].copy_(p.tok_inst.clamp(min=0))
        for t in range(M):
            dl = md.dim_latents[t]
            capi.check(ode_stage(Y.data_ptr(), Ym.data_ptr(), p.ctl.data_ptr(), B, Lc, dmax, p.lat[t]['x'].data_ptr(), H, Lq, dl, unit_blk0, sp), 'tfx_ode_stage')
        self._pos_emb_rows(p, lay, r, states)
        self._run(p, stream, 0, p.fwd_cond[0])
        self._run(p, stream, p.fwd_cond[1], p.fwd_pred_end)
        for t in range(M):
            dl = md.dim_latents[t]
            capi.check(ode_update(Y.data_ptr(), Ym.data_ptr(), *hist, p.ctl.data_ptr(), B, Lc, dmax, p.lat[t]['pred'].data_ptr(), H, Lq, dl,
                                  float(c.cfg_scale), blocks.sel[t].data_ptr() if M > 1 else None, unit_blk0, sp), 'tfx_ode_update')

    def _upload_row_maps(self, p, lay, r, ctl):
        """row maps of all types + the solver control block (per sample: the mode - 1 / 2 of `ctl`, 3 = a finished block goes in, 0 = none - and the
        rows of `ctl` at the sample's evaluation): one staging buffer, one copy"""
        M, B = self.m.num_modalities, r.is_m.size
        hb = self._pinned('rowbuf', (p.rowbuf.numel(),), torch.int32)
        hv = hb.numpy()
        rs, T = p.row_stride, lay.blk_rows.size
        rowidx = np.arange(T, dtype=np.int32)
        for t in range(M):
            mine = lay.blk_rows if M == 1 else lay.blk_rows & (lay.row_ty == t)
            hv[t * rs:t * rs + T] = np.where(mine, rowidx, -1)
            hv[(M + t) * rs:(M + t) * rs + T] = np.where(mine, rowidx, 0)
        cw = hv[2 * M * rs:].view(np.float32)
        kk = np.minimum(r.k, len(ctl.times) - 1)
        cw[:B] = np.where(r.is_m, ctl.modes[kk], np.where(r.com, 3., 0.))
        cw[B:(1 + len(ctl.rows)) * B] = np.where(r.is_m, ctl.rows[:, kk], 0.).reshape(-1)
        p.rowbuf.copy_(hb, non_blocking=True)

    def _pos_emb_rows(self, p, lay, r, states):
        """blocks that carry their axial positional embedding: a finished one always (history-style, T:3173-3176), one being decoded under `pos_emb_in_decode`"""
        B, H = r.is_m.size, r.base.shape[0]
        for t in p.ext_add:
            add = p.lat[t]['add']
            add.zero_()
            for i in np.flatnonzero((r.is_m & bool(self.pos_emb_in_decode)) | r.com):
                if states[i].curr_modality_id != t:
                    continue
                rows = self.m._pos_rows(t, [states[i].modality_shape])
                for h in range(H) if r.is_m[i] else [1]:
                    lo = int(lay.unit_row0[h * B + i])
                    add[lo:lo + rows.shape[0]].copy_(rows)

    def _advance(self, states, toks, blocks, n_evals, c):
        """every live sample moves on by what the step did for it: its fed token is cached and the sampled one accepted, or one more evaluation is done"""
        eos_id, max_length, lockstep = self.m.eos_id, c.max_length, c.use_cfg
        live = np.flatnonzero(blocks.A[PH])
        for i in live:
            st = states[i]
            if st.phase == 'text':
                st.fed(lockstep)
                if st.accept(toks[i], eos_id, max_length) and self._maybe_transition(st, c.fixed_shape):
                    blocks.begin(i, st)
            else:
                if st.som_pending:
                    st.som_fed()
                st.ode_k += 1
                if st.ode_k == n_evals:
                    self._commit(st, blocks.Y[i], c, lockstep)
        blocks.mirror(states, live)

    # ------------------------------------------------------------------ phased schedule (the reference's loop, T:2226-2360)
    def _loop_phased(self, states, joint, c):
        while not all(s.phase == 'done' for s in states):
            joint = self._text_rounds(states, joint, c)
            group = [i for i, s in enumerate(states) if s.phase == 'modality']
            if group:
                joint = self._joint_ode(states, group, joint, c)

    def _text_rounds(self, states, joint, c):
        """text steps over the conditional cache until no sample is in its text phase"""
        md, B = self.md, c.B
        while any(s.phase == 'text' for s in states):
            joint = self._ensure_capacity(joint, states, 1); cache = joint[:, :B]
            p = self._decode_plan(('text', cache.data_ptr()), B, 1, cache, False)
            ids = np.zeros(B, np.int32); pos = np.full(B, -1, np.int32); kve = np.ones(B, np.int32); rot = np.zeros(B, np.int32)
            for i, st in enumerate(states):
                kve[i] = max(st.cache_len, 1)
                if st.phase == 'text':
                    ids[i], pos[i], kve[i], rot[i] = st.last_token, i * cache.shape[2] + st.cache_len, st.cache_len + 1, st.tokens_seen
            self._load(p, ids=ids, pos=pos, kve=kve, rot=rot, tok_inst=np.full(B, -1, np.int32))
            self._run(p, c.stream, 0, p.fwd_logits_end)
            toks = _sample_text_token(p.logits, md.vocab, c.temperature, c.min_p, c.stream, c.top_k, c.top_p).tolist()
            for st, tok in zip(states, toks):
                if st.phase == 'text':
                    st.fed(False)
                    if st.accept(tok, self.m.eos_id, c.max_length):
                        self._maybe_transition(st, c.fixed_shape)
        return joint

    def _uncond_history(self, states, group, joint, Lmax, c):
        """the null-text cache of the samples in `group` up to date with their histories (T:2386-2406), with room for a block of Lmax rows"""
        B = c.B
        if os.environ.get('TFX_UNCOND_INCREMENTAL', '1') != '0' and all(states[i].uncond_parts > 0 for i in group):
            # the reference re-runs the whole null-text history before every modality (T:2386-2406).  Its keys / values for the part
            # already in the cache do not change, so only what each sample appended since its last modality - the decoded block
            # (conditioned at t = 1) and the text after it - goes through the model, as ONE multi-token decode step against the cache
            need = max(_flat_len(states[i].parts) for i in group) + Lmax + 8
            if joint.shape[2] < need:
                joint = self._grow(joint, need)
            self._uncond_append(states, group, joint[:, B:], c.stream)
            return joint
        hist = [states[i].parts if i in group else [[self.m.null_text_id]] for i in range(B)]
        return self._uncond_prefill(joint, states, hist, group, Lmax + 8)

    def _joint_ode(self, states, group, joint, c):
        """the modality phase: the blocks of all samples in `group` decoded by one joint solve, then committed"""
        md, dev, B = self.md, self.dev, c.B
        Lmax = max(states[i].modality_length for i in group)
        joint = self._ensure_capacity(joint, states, Lmax)
        if c.use_cfg:
            joint = self._uncond_history(states, group, joint, Lmax, c)
        y = torch.zeros(B, Lmax, max(md.dim_latents), device=dev)
        for i in group:
            self._init_noise(y[i], states[i], c)
        nb = c.H * B
        jp = self._decode_plan(('mod', nb, Lmax, joint.data_ptr()), nb, Lmax, joint, True)
        self._load_modality(jp, states, group, Lmax, joint.shape[2], halves=c.H)
        type_mask = self._type_masks(states, group, Lmax)
        if c.use_cfg:
            type_mask = {ty: torch.cat([mk, mk]) for ty, mk in type_mask.items()}

        def velocity(t, x):
            """the conditional and the null-text evaluation in one forward (rows [0, B) and [B, 2B))"""
            if not c.use_cfg:
                return self._eval(jp, type_mask, Lmax, t, x, c.stream), None
            out = self._eval(jp, type_mask, Lmax, t, torch.cat([x, x]), c.stream)
            return out[:B], out[B:]

        y = _ode_solve(self.m.ode_method, c.modality_steps, y, velocity, c.cfg_scale, c.stream)
        for i in group:
            self._commit(states[i], y[i], c, False)
        return joint

    # ------------------------------------------------------------------ pure-text generation (T:2666-2707)
    def generate_text_only(self, prompt, seq_len, temperature, min_p, top_k=None, top_p=None):
        """KV-cached greedy / min-p sampling of text only: prefill the prompt once, then one-token decode plans.
        Mirrors the reference exactly: temperature 0 takes the argmax over ALL logits, otherwise min-p filter, then the
        text-only mask (T:2690-2698)."""
        m, md, dev = self.m, self.md, self.dev
        m._require_gpu()
        prompt = prompt.to(dev)
        B, n0 = prompt.shape
        num = max(0, seq_len - n0)
        out = torch.empty(B, num, dtype=torch.long, device=dev)
        if num == 0:
            return out
        stream = m._stream()
        pick = lambda logits: _pick_text_only(logits, md.vocab, m.num_text_tokens, temperature, min_p, stream, top_k, top_p)
        plan, S = m._forward_plain([[row] for row in prompt], torch.ones(B, 1, device=dev), add_meta=False)
        n_pad = S['n']
        maxlen = (max(n_pad, n0 + num) + 64) // 64 * 64
        m._decode_plans = {}
        cache = self._alloc_cache(B, maxlen)
        self._fill_cache(cache, plan, B, n_pad)
        tok = pick(plan.logits.view(B, n_pad, md.vp)[:, n0 - 1].contiguous())
        out[:, 0] = tok
        p = self._decode_plan(('text', cache.data_ptr()), B, 1, cache, False)
        rows = np.arange(B, dtype=np.int32) * maxlen
        for step in range(1, num):
            L = n0 + step - 1                                          # keys already in the cache
            self._load(p, ids=tok.to(torch.int32).cpu().numpy(), pos=rows + L, kve=np.full(B, L + 1, np.int32), rot=np.full(B, L, np.int32),
                       tok_inst=np.full(B, -1, np.int32))
            self._run(p, stream, 0, p.fwd_logits_end)
            tok = pick(p.logits)
            out[:, step] = tok
        return out

    def _uncond_append(self, states, group, ucache, stream):
        """append what the samples of `group` added to their histories since their last modality phase - parts[uncond_parts:] : modality blocks
        (prompt-style: conditioned at t = 1, bidirectional inside the block, one rotary position) and text (every integer token as the null id,
        causal) - to the null-text KV cache with one decode-style forward; rows / positions as packing.token_maps would lay the full history out"""
        m, md, B = self.m, self.md, len(states)
        segs = {i: states[i].parts[states[i].uncond_parts:] for i in group}
        Lq = max(8, -(-max(_flat_len(v) for v in segs.values()) // 8) * 8)         # bucketed: a handful of plans
        assert all(sum(isinstance(p, tuple) for p in v) <= 1 for v in segs.values()), 'one decoded modality per sample between two phases'
        maxlen = ucache.shape[2]
        p = self._decode_plan(('uinc', Lq, ucache.data_ptr()), B, Lq, ucache, True)
        T = B * Lq
        ids = np.zeros(T, np.int32); pos = np.full(T, -1, np.int32); kve = np.ones(T, np.int32); rot = np.zeros(T, np.int32)
        tok_inst = np.full(T, -1, np.int32)
        row_tok = {t: np.full(T, -1, np.int32) for t in range(m.num_modalities)}
        for t in p.ext_add:
            p.lat[t]['add'].zero_()
        for i in range(B):
            st = states[i]
            kve[i * Lq:(i + 1) * Lq] = max(st.uncond_len, 1)
            if i not in segs:
                continue
            j, rp = 0, st.uncond_pos
            for part in segs[i]:
                if isinstance(part, tuple):
                    ty, x = part
                    L = math.prod(x.shape[:-1])
                    sl = slice(i * Lq + j, i * Lq + j + L)
                    pos[sl] = i * maxlen + st.uncond_len + j + np.arange(L)
                    kve[sl] = st.uncond_len + j + L                       # the whole block sees itself
                    rot[sl] = rp; rp += 1
                    tok_inst[sl] = i
                    row_tok[ty][sl] = np.arange(i * Lq + j, i * Lq + j + L)
                    p.lat[ty]['x'][i * Lq + j:i * Lq + j + L].copy_(x.reshape(L, -1))
                    if ty in p.ext_add:                                   # history modalities carry their positional embedding (T:3173-3176)
                        p.lat[ty]['add'][i * Lq + j:i * Lq + j + L].copy_(m._pos_rows(ty, [tuple(x.shape[:-1])]))
                    j += L
                else:
                    n = len(part)
                    sl = slice(i * Lq + j, i * Lq + j + n)
                    ids[sl] = m.null_text_id
                    pos[sl] = i * maxlen + st.uncond_len + j + np.arange(n)
                    kve[sl] = st.uncond_len + j + 1 + np.arange(n)
                    rot[sl] = rp + np.arange(n); rp += n
                    j += n
            st.null_appended(j, rp)
        self._load(p, ids, pos, kve, rot, tok_inst)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        for t in row_tok:
            p.row_tok[t].copy_(up(row_tok[t])); p.row_src[t].copy_(up(np.maximum(row_tok[t], 0)))
            p.row_inst[t].copy_(up(np.repeat(np.arange(B, dtype=np.int32), Lq)))
            p.set_noise(t, None)
        p.inst_time.fill_(1.)
        self._run(p, stream, 0, p.fwd_embed_end)

    def _ensure_capacity(self, cache, states, extra):
        need = max(s.cache_len for s in states) + extra + 1
        return cache if need <= cache.shape[2] else self._grow(cache, need + 192)

    def _grow(self, cache, need):
        new = self._alloc_cache(cache.shape[1], (need + 63) // 64 * 64)
        new[:, :, :cache.shape[2]].copy_(cache)
        self.m._decode_plans = {}
        self._grew = True
        return new

    def _load(self, p, ids, pos, kve, rot, tok_inst, units=None):
        """the step's five index arrays go up in ONE pinned, asynchronous copy (rows 0..4 of Plan.idx): no host sync, no pageable staging"""
        T = p.T
        rows = 5 if units is None else 7                                 # compacted plans: the per-sample arrays ride in row 6 (row 5, q_start, stays zero)
        host = self._pinned('idx', (rows, p.idx.shape[1]), torch.int32, zero=True)
        hv = host.numpy()
        hv[0, :T], hv[1, :T], hv[2, :T], hv[3, :T], hv[4, :T] = ids, pos, kve, rot, tok_inst
        if units is not None:
            hv[6, :units.size] = units
        p.idx[:rows].copy_(host, non_blocking=True)
        p.set_rope_tables(*self.m._rope_tables(int(rot.max()) + 1))

    def _load_modality(self, p, states, group, Lmax, maxlen, halves=1):
        """index arrays of a modality decode step.  halves = 2: rows [0, B) run against the real history, rows [B, 2B) against the null-text
        history (second half of the joint cache, its own prefix lengths) - the two evaluations of classifier-free guidance in one forward"""
        B, md = len(states), self.md
        T = halves * B * Lmax
        ids = np.zeros(T, np.int32); pos = np.full(T, -1, np.int32); kve = np.ones(T, np.int32); rot = np.zeros(T, np.int32)
        tok_inst = np.full(T, -1, np.int32)
        row_tok = {t: np.full(T, -1, np.int32) for t in range(self.m.num_modalities)}
        for h in range(halves):
            for i in range(B):
                st = states[i]
                r = h * B + i                                              # batch row of the plan = cache row
                base = st.uncond_len if h == 1 else st.cache_len
                kve[r * Lmax:(r + 1) * Lmax] = max(base, 1)
                if i not in group:
                    continue
                L, ty = st.modality_length, st.curr_modality_id
                sl = slice(r * Lmax, r * Lmax + L)
                kve[r * Lmax:(r + 1) * Lmax] = base + L                    # own prefix + own (bidirectional) modality block, T:2415-2419
                pos[sl] = r * maxlen + base + np.arange(L)
                rot[r * Lmax:(r + 1) * Lmax] = st.tokens_seen              # every token of the instance shares one position, T:2411
                tok_inst[sl] = r
                row_tok[ty][sl] = np.arange(r * Lmax, r * Lmax + L)
        self._load(p, ids, pos, kve, rot, tok_inst)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        for t in row_tok:
            p.row_tok[t].copy_(up(row_tok[t])); p.row_src[t].copy_(up(np.maximum(row_tok[t], 0)))
            p.row_inst[t].copy_(up(np.repeat(np.arange(halves * B, dtype=np.int32), Lmax)))
            p.set_noise(t, None)
        for t in p.ext_add:                      # axial positional embedding of the blocks being decoded (constant over the ODE steps); zeros = none
            add = p.lat[t]['add']
            add.zero_()
            if self.pos_emb_in_decode:
                for h in range(halves):
                    for i in group:
                        st = states[i]
                        if st.curr_modality_id == t:
                            r = h * B + i
                            add[r * Lmax:r * Lmax + st.modality_length].copy_(self.m._pos_rows(t, [st.modality_shape]))

    def _run(self, p, stream, lo, hi):
        """replay a range of a decode plan: eagerly the first time (one-off kernel attribute setup happens outside any capture), as a
        hipGraph afterwards - every kernel argument of a decode plan is a fixed pointer, the per-step values live in device arrays"""
        seen = p.__dict__.setdefault('_ran', set())
        if (lo, hi) not in seen:
            seen.add((lo, hi))
            Plan.run(p.fwd, stream, lo, hi)
        else:
            Plan.run(p.fwd, stream, lo, hi, graph=True)

    def _type_masks(self, states, group, Lmax):
        """per modality type: (B, Lmax, 1) 0/1 mask of the state rows that belong to a sample decoding that type"""
        B = len(states)
        masks = {}
        for ty in range(self.m.num_modalities):
            mk = np.zeros((B, Lmax, 1), np.float32)
            for i in group:
                if states[i].curr_modality_id == ty:
                    mk[i, :states[i].modality_length] = 1.
            masks[ty] = torch.from_numpy(mk).to(self.dev)
        return masks

    def _eval(self, p, type_mask, Lmax, t, y, stream):
        """one model evaluation of the joint ODE state y (B, Lmax, dmax) at time t -> predicted flow, same layout (T:2468-2521)."""
        md, B = self.md, y.shape[0]
        p.inst_time.fill_(t)
        for ty in range(self.m.num_modalities):
            p.lat[ty]['x'].copy_(y[:, :, :md.dim_latents[ty]].reshape(B * Lmax, md.dim_latents[ty]))
        self._run(p, stream, 0, p.fwd_embed_end)
        self._run(p, stream, p.fwd_logits_end, p.fwd_pred_end)
        if self.m.num_modalities == 1 and md.dim_latents[0] == y.shape[2]:
            return p.lat[0]['pred'].view(B, Lmax, -1) * type_mask[0]
        out = torch.zeros_like(y)
        for ty in range(self.m.num_modalities):
            dl = md.dim_latents[ty]
            out[:, :, :dl] += p.lat[ty]['pred'].view(B, Lmax, dl) * type_mask[ty]
        return out
