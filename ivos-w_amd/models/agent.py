"""Double-DQN frame-recommendation agent on the MI355X — drop-in for the reference's ``models.agent``.

Same class surface as /root/reference/models/agent.py (``Brain`` :13-64, ``Agent`` :67-236), with the
arithmetic replaced by libivosw_hip.so:

  Brain.forward        -> ivosw_brain_forward   (batched encoder/gate GEMMs + register-resident LSTM recurrence)
  Agent.update_agent   -> ivosw_dqn_loss_grad_ex (3 forwards, two-term Double-DQN loss: the reference's MSE, or Huber with
                                                  cfg.agent.loss = "huber" / huber_delta; hand-derived BPTT)
                          [+ RCCL all-reduce of the flat gradient arena when torch.distributed is up]
                          ivosw_clamp_adam       (clamp [-1,1] + coupled-L2 Adam, one fused kernel; cfg.agent.optimizer = "sgd":
                          ivosw_clamp_sgd         clamp + SGD with momentum / nesterov, cfg.agent.momentum / nesterov;
                                                  cfg.agent.lr_schedule = "poly": the lr of each update from a table, see poly_lr_table)
                          ivosw_copy_f32         (hard target sync on the reference's host coin, cfg.agent.target_update = "coin";
                          ivosw_target_update     "soft" / "periodic": the rule on the device, fused into the one-call step's last launch)
  Agent.action         -> ivosw_brain_forward + ivosw_brain_argmax (first max, like numpy)
  Agent.actions        -> ivosw_brain_forward_ragged + ivosw_brain_argmax_ragged (several states of different lengths, one launch chain)
  cfg.agent.candidates / skip_annotated -> ivosw_brain_topk_ragged in the argmax's place (k ranked frames per state, annotated ones last)
  cfg.agent.candidate_gap > 1 -> ivosw_brain_topk_spread_ragged in its place (the k frames at least that many frames apart, greedily)

torch modules (nn.Linear / nn.LSTMCell) are used only as parameter containers so that ``state_dict()`` keys,
shapes and default initialisation are the reference's; their ``forward`` is never called.  All ten tensors are
views into one flat fp32 arena (``Brain.flat``), which is what the C ABI, the optimizer and the all-reduce operate on.
"""
import math
import random

import numpy as np
import torch
import torch.nn as nn

from .. import _lib as L
from .momory_pool import PrioritizedReplay, ReplayMemory, per_params

_ORDER = ("encoder_fc1.weight", "encoder_fc1.bias", "encoder_fc2.weight", "encoder_fc2.bias",
          "lstm_cell.weight_ih", "lstm_cell.weight_hh", "decoder_fc1.weight", "decoder_fc1.bias",
          "decoder_fc2.weight", "decoder_fc2.bias")


def _adjacent_rows(states):
    """The flat [R,2] tensor behind ``states`` when they are consecutive row slices of ONE contiguous fp32 [*,2] tensor, else None."""
    base = states[0]._base if torch.is_tensor(states[0]) else None
    if base is None or base.dim() != 2 or base.shape[1] != 2 or base.dtype != torch.float32 or not base.is_contiguous():
        return None
    first = states[0].storage_offset() - base.storage_offset()
    want = first
    for s in states:
        if not torch.is_tensor(s) or s._base is not base or s.dim() != 2 or s.shape[1] != 2 or not s.is_contiguous() \
                or s.storage_offset() - base.storage_offset() != want:
            return None
        want += 2 * s.shape[0]
    if first % 2:
        return None
    return base[first // 2:want // 2]


class Brain(nn.Module):
    def __init__(self, lstm_input_channels=128, hidden_channels=128, num_fc_concat=128):
        super().__init__()
        if (lstm_input_channels, hidden_channels, num_fc_concat) != (128, 128, 128):
            raise ValueError("the HIP Brain is specialised for the reference's 128/128/128 widths")
        self.input_channels, self.hidden_channels, self.num_fc_concat = 128, 128, 128
        # parameter containers, created in the reference's order so a seeded init matches it
        self.encoder_fc1 = nn.Linear(2, 128)
        self.encoder_fc2 = nn.Linear(128, 128)
        self.lstm_cell = nn.LSTMCell(128, 128, False)
        self.decoder_fc1 = nn.Linear(256, 128)
        self.decoder_fc2 = nn.Linear(128, 1)
        self.flat = None
        self.flat_grad = None
        self._ws = L.Workspace()
        self._pack()

    # ------------------------------------------------------------------ flat arena
    def _named(self):
        table = dict(self.named_parameters())
        return [table[k] for k in _ORDER]

    def _pack(self):
        """(Re)build the flat arena and make every parameter (and its .grad) a view into it."""
        params = self._named()
        dev = params[0].device
        flat = torch.empty(L.BRAIN_NPARAMS, dtype=torch.float32, device=dev)
        grad = torch.zeros(L.BRAIN_NPARAMS, dtype=torch.float32, device=dev)
        off = 0
        for p in params:
            n = p.numel()
            flat[off:off + n].copy_(p.data.reshape(-1).float())
            p.data = flat[off:off + n].view(p.shape)
            p.grad = grad[off:off + n].view(p.shape)
            off += n
        assert off == L.BRAIN_NPARAMS
        self.flat, self.flat_grad = flat, grad

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self._pack()
        return out

    # ------------------------------------------------------------------ forward
    def forward(self, input):
        """input [N,T,2] -> Q [N,T].  Inference only (the DQN update has its own fused backward)."""
        x = input.detach().to(dtype=torch.float32).contiguous()
        N, T, P = x.shape
        assert P == 2
        q = torch.empty(N, T, dtype=torch.float32, device=x.device)
        lib = L.lib()
        nbytes = lib.ivosw_brain_ws_bytes(N, T)
        ws = self._ws.get(nbytes, x.device)
        L.check(lib.ivosw_brain_forward(L.dptr(self.flat), L.dptr(x), N, T, L.dptr(q), L.dptr(ws), nbytes,
                                        L.stream_ptr(x.device)), "brain_forward")
        return q

    def forward_ragged(self, states, lengths=None):
        """Q of SEVERAL sequences, each of its own length, in one launch chain (ivosw_brain_forward_ragged).  ``states`` is a sequence of
        [T_k,2] fp32 tensors on this network's device, or ONE flat [R,2] tensor with ``lengths`` (R = their sum).  Returns (q, views): the
        flat Q [R] and one [T_k] view of it per sequence.  Each view holds, bit for bit, ``forward(state[None])[0]`` of its sequence:
        nothing is padded, the backward direction of every sequence starts at its own last frame.  More than 128 sequences run in
        groups of 128."""
        if lengths is None:
            states = list(states)
            lengths = [int(s.shape[0]) for s in states]
            if not states:
                raise ValueError("forward_ragged needs at least one sequence")
            x = _adjacent_rows(states)                        # slices of one flat [R,2] tensor, in order: read in place
            if x is None:
                x = states[0] if len(states) == 1 else torch.cat([s.detach().to(dtype=torch.float32) for s in states], 0)
        else:
            x, lengths = states, [int(n) for n in lengths]
        x = x.detach().to(dtype=torch.float32).contiguous()
        if x.dim() != 2 or x.shape[1] != 2 or not lengths or min(lengths) < 1 or sum(lengths) != x.shape[0]:
            raise ValueError(f"forward_ragged: states must be [R,2] with positive lengths that sum to R, got {tuple(x.shape)} and {lengths}")
        q = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
        self.forward_ragged_into(x, lengths, q)
        views, off = [], 0
        for n in lengths:
            views.append(q[off:off + n])
            off += n
        return q, views

    def forward_ragged_into(self, x, lengths, q):
        """forward_ragged on a flat contiguous fp32 x [R,2] into a preallocated q [R] (no allocation beyond the grow-only workspace)."""
        lib, off = L.lib(), 0
        for g in range(0, len(lengths), L.MAX_SEQS):
            group = lengths[g:g + L.MAX_SEQS]
            arr = L.int_array(group)
            rows = int(lib.ivosw_brain_ragged_rows(arr, len(group)))
            if rows < 0:
                L.check(rows, "brain_ragged_rows")
            nbytes = lib.ivosw_brain_ragged_ws_bytes(rows)
            ws = self._ws.get(nbytes, x.device)
            L.check(lib.ivosw_brain_forward_ragged(L.dptr(self.flat), L.dptr(x[off:off + rows]), arr, len(group), L.dptr(q[off:off + rows]),
                                                   L.dptr(ws), nbytes, L.stream_ptr(x.device)), "brain_forward_ragged")
            off += rows
        return q


LR_SCHEDULES = ("constant", "poly")
LR_TOTAL_STEPS_MAX = 1 << 24          # the poly schedule's table: N + 1 float32 values on the device, 64 MB at the cap


def lr_schedule_option(kind, lr_pow, total_steps):
    """(schedule, lr_pow, N), checked: ("constant", None, None), or ("poly", lr_pow, N) with lr_pow a finite number >= 0 and N an int in
    [1, LR_TOTAL_STEPS_MAX].  lr_pow and N are only looked at under "poly".  Anything else is a ValueError."""
    if not isinstance(kind, str) or kind not in LR_SCHEDULES:
        raise ValueError(f"agent.lr_schedule must be 'constant' or 'poly', got {kind!r}")
    if kind == "constant":
        return "constant", None, None
    if isinstance(total_steps, bool) or not isinstance(total_steps, int) or not 1 <= total_steps <= LR_TOTAL_STEPS_MAX:
        raise ValueError(f"agent.lr_total_steps must be an int in [1, {LR_TOTAL_STEPS_MAX}] under lr_schedule 'poly', got {total_steps!r}")
    if isinstance(lr_pow, bool) or not isinstance(lr_pow, (int, float)) or not (math.isfinite(lr_pow) and lr_pow >= 0):
        raise ValueError(f"agent.lr_pow must be a finite number >= 0, got {lr_pow!r}")
    return "poly", float(lr_pow), total_steps


REPLAYS = ("uniform", "prioritized")


def replay_option(kind, alpha=0.6, beta0=0.4, beta_steps=0, eps=1e-6):
    """(replay, alpha, beta0, N_beta, eps), checked: ("uniform", None, None, None, None) - today's minibatches, the PER values not looked
    at - or ("prioritized", alpha, beta0, N_beta, eps) with alpha finite >= 0, beta0 in [0, 1], N_beta an int >= 0 and eps finite > 0
    (momory_pool.per_params).  Anything else is a ValueError."""
    if not isinstance(kind, str) or kind not in REPLAYS:
        raise ValueError(f"agent.replay must be 'uniform' or 'prioritized', got {kind!r}")
    if kind == "uniform":
        return "uniform", None, None, None, None
    return ("prioritized",) + per_params(alpha, beta0, beta_steps, eps)


def poly_lr_table(lr, lr_pow, total_steps):
    """lr_k = float32(lr * (1 - min(k, N) / N) ** lr_pow) for k = 0 .. N (torch's PolynomialLR closed form at last_epoch = k): float64
    Python arithmetic (libm pow; not numpy's vectorised power, whose last bit can differ), rounded to float32 once at the end."""
    lr, n = float(lr), int(total_steps)
    return np.array([lr * (1.0 - k / n) ** lr_pow for k in range(n + 1)], dtype=np.float64).astype(np.float32)


TARGET_UPDATES = ("coin", "soft", "periodic")
_TARGET_MODES = {"soft": L.TARGET_SOFT, "periodic": L.TARGET_PERIODIC}


def target_update_option(kind, tau=0.005, period=20):
    """(target_update, tau, period), checked: ("coin", None, None) - the reference's host coin, tau and period not looked at -, ("soft",
    tau, None) with tau a number in the open interval (0, 0.5), or ("periodic", None, period) with period an int in [1, 2**31 - 1].
    Anything else is a ValueError."""
    if not isinstance(kind, str) or kind not in TARGET_UPDATES:
        raise ValueError(f"agent.target_update must be 'coin', 'soft' or 'periodic', got {kind!r}")
    if kind == "coin":
        return "coin", None, None
    if kind == "soft":
        if isinstance(tau, bool) or not isinstance(tau, (int, float)) or not 0 < tau < 0.5 or not 0 < float(np.float32(tau)) < 0.5:
            raise ValueError(f"agent.tau must be a number in the open interval (0, 0.5), got {tau!r} (torch's lerp changes formula at 0.5; "
                             "for hard copies use agent.target_update='periodic' with agent.target_period)")
        return "soft", float(tau), None
    if isinstance(period, bool) or not isinstance(period, int) or not 1 <= period < 2 ** 31:
        raise ValueError(f"agent.target_period must be an int in [1, 2**31 - 1], got {period!r}")
    return "periodic", None, period


def target_update_mirror(target, policy, kind, tau=None, period=None, k=1):
    """Host mirror of ivosw_target_update: the float32 target after step k (counted from 1) given the float32 policy after that step's
    update.  soft: fmaf(float32(tau), p - t, t) with ONE rounding - the product-sum is formed in float64 rounded to odd (an error-free
    two-sum decides the sticky bit), which the final rounding to float32 turns into the correctly rounded result.  periodic: a copy of
    the policy when k % period == 0, the target unchanged otherwise."""
    t, p = np.asarray(target, dtype=np.float32), np.asarray(policy, dtype=np.float32)
    if kind == "periodic":
        return p.copy() if k % period == 0 else t.copy()
    if kind != "soft":
        raise ValueError(f"no device rule for target_update {kind!r}")
    a = np.float64(np.float32(tau)) * (p - t).astype(np.float64)          # exact: 24 x 24 bits
    b = t.astype(np.float64)
    s = a + b
    bb = s - a
    err = (a - (s - bb)) + (b - bb)                                         # two-sum: a + b == s + err exactly
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0) & even
    toward = np.where((err > 0), np.inf, -np.inf)
    s = np.where(fix, np.nextafter(s, toward), s)                           # round to odd
    return s.astype(np.float32)


class _LrSchedule:
    """The learning-rate schedule of FusedClampAdam and FusedClampSGD.  ``param_groups[0]`` carries ``lr_schedule`` ("constant" or
    "poly"), ``lr_pow`` and ``lr_total_steps`` next to the base ``lr``.  Under "poly" the update after k earlier ones uses
    ``poly_lr_table(lr, lr_pow, N)[min(k, N)]``: the eager entries get that float as their lr, and the captured and one-call steps read the
    same table on the device at their device step counter.  Under "constant" every path passes ``lr`` as before."""

    def _init_schedule(self, lr_schedule, lr_pow, lr_total_steps):
        kind, lr_pow, n = lr_schedule_option(lr_schedule, lr_pow, lr_total_steps)
        self.param_groups[0].update(lr_schedule=kind, lr_pow=lr_pow, lr_total_steps=n)
        self._lr_host = None                    # ((lr, lr_pow, N), the host table) of the schedule in use
        self._lr_dev = {}                       # (lr, lr_pow, N, device) -> device table; kept, so that a captured graph's stays valid

    def schedule(self):
        """(schedule, base lr, lr_pow, N) as param_groups[0] holds them now (checked)."""
        g = self.param_groups[0]
        kind, lr_pow, n = lr_schedule_option(g.get("lr_schedule", "constant"), g.get("lr_pow"), g.get("lr_total_steps"))
        return kind, float(g["lr"]), lr_pow, n

    @property
    def scheduled(self):
        return self.schedule()[0] == "poly"

    def _lr_table_host(self):
        _, lr, lr_pow, n = self.schedule()
        if self._lr_host is None or self._lr_host[0] != (lr, lr_pow, n):
            self._lr_host = ((lr, lr_pow, n), poly_lr_table(lr, lr_pow, n))
        return self._lr_host[1]

    def lr_table(self):
        """The poly table on the parameters' device (float32 [N + 1]), built once per (lr, lr_pow, N) and device and kept for the
        optimizer's life: a captured step records its address."""
        host = self._lr_table_host()
        dev = self.brain.flat.device
        key = self._lr_host[0] + (str(dev),)
        t = self._lr_dev.get(key)
        if t is None:
            t = self._lr_dev[key] = torch.from_numpy(host).to(dev)
        return t

    def lr_at(self, k):
        """The lr of the update that follows k earlier ones."""
        kind, _, _, n = self.schedule()
        if kind == "constant":
            return self.param_groups[0]["lr"]
        return float(self._lr_table_host()[min(int(k), n)])

    def current_lr(self):
        """The lr the next update will use."""
        return self.lr_at(self.state["step"])

    def _schedule_hyper(self):
        """What a captured step bakes in of the schedule: its kind, lr_pow, N and the device table's address (the base lr is in hyper())."""
        kind, _, lr_pow, n = self.schedule()
        return (kind, lr_pow, n, self.lr_table().data_ptr() if kind == "poly" else 0)

    def _load_schedule(self, sd):
        """The schedule of a state dict's param_groups, when it carries one (checked before anything is changed)."""
        groups = sd.get("param_groups") or [{}]
        if "lr_schedule" in groups[0]:
            g = groups[0]
            kind, lr_pow, n = lr_schedule_option(g["lr_schedule"], g.get("lr_pow"), g.get("lr_total_steps"))
            self.param_groups[0].update(lr_schedule=kind, lr_pow=lr_pow, lr_total_steps=n)


class FusedClampAdam(_LrSchedule):
    """``optim.Adam(params, lr, weight_decay)`` + the reference's grad clamp, as one kernel over the flat arena.

    The interface CapturedDqnStep and parallel.py use, shared with FusedClampSGD: ``kind``, ``step``, ``dev_state`` (the device state a
    captured step needs, created and synchronised), ``enqueue_dev_step`` (the capture-safe update on the current stream), ``note_dev_steps``
    (the host counter after n such updates), ``hyper`` (what a capture bakes in), ``onecall_tail`` (the one-call step's entry and the
    arguments after its ws_bytes) and the learning-rate schedule of _LrSchedule."""

    kind = "adam"

    def __init__(self, brain, lr, weight_decay, betas=(0.9, 0.999), eps=1e-8, clamp=1.0, lr_schedule="constant", lr_pow=None,
                 lr_total_steps=None):
        self.brain = brain
        self.param_groups = [dict(params=list(brain.parameters()), lr=lr, betas=betas, eps=eps,
                                  weight_decay=weight_decay, clamp=clamp)]
        self._init_schedule(lr_schedule, lr_pow, lr_total_steps)
        self.state = dict(step=0, exp_avg=None, exp_avg_sq=None)
        self.grad_scale = 1.0

    def _ensure(self):
        flat = self.brain.flat
        if self.state["exp_avg"] is None or self.state["exp_avg"].device != flat.device:
            self.state["exp_avg"] = torch.zeros_like(flat)
            self.state["exp_avg_sq"] = torch.zeros_like(flat)

    def zero_grad(self, set_to_none=False):
        self.brain.flat_grad.zero_()

    def step(self):
        self._ensure()
        g = self.param_groups[0]
        lr = self.current_lr()
        self.state["step"] += 1
        b = self.brain
        L.check(L.lib().ivosw_clamp_adam(L.dptr(b.flat), L.dptr(b.flat_grad), L.dptr(self.state["exp_avg"]),
                                         L.dptr(self.state["exp_avg_sq"]), L.BRAIN_NPARAMS, self.state["step"],
                                         lr, g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"],
                                         g["clamp"], self.grad_scale, L.stream_ptr(b.flat.device)), "clamp_adam")

    # -- device-side step state (what a captured HIP graph replays; ivosw_clamp_adam_dev) -------------------------------
    def dev_state(self):
        """The 32-byte Adam step state on the device, (re)synchronised with the host step counter (and the schedule's table, when on)."""
        self._ensure()
        if self.scheduled:
            self.lr_table()
        dev = self.brain.flat.device
        ds = self.state.get("dev")
        if ds is None or ds.device != dev:
            ds = torch.zeros(L.lib().ivosw_adam_state_bytes(), dtype=torch.uint8, device=dev)
            self.state["dev"], self.state["dev_step"] = ds, 0
        if self.state["dev_step"] != self.state["step"]:
            ds[16:20].copy_(torch.from_numpy(np.array([self.state["step"]], dtype=np.int32).view(np.uint8)))
            self.state["dev_step"] = self.state["step"]
        return ds

    def enqueue_dev_step(self):
        """ivosw_clamp_adam_dev (ivosw_clamp_adam_dev_sched on the poly schedule) on the current stream (inside a capture: recorded); the
        caller bumps the host counter per replay."""
        g, b = self.param_groups[0], self.brain
        if self.scheduled:
            L.check(L.lib().ivosw_clamp_adam_dev_sched(L.dptr(b.flat), L.dptr(b.flat_grad), L.dptr(self.state["exp_avg"]),
                                                       L.dptr(self.state["exp_avg_sq"]), L.BRAIN_NPARAMS, L.dptr(self.state["dev"]),
                                                       L.dptr(self.lr_table()), self.schedule()[3], g["betas"][0], g["betas"][1], g["eps"],
                                                       g["weight_decay"], g["clamp"], self.grad_scale, L.stream_ptr(b.flat.device)),
                    "clamp_adam_dev_sched")
            return
        L.check(L.lib().ivosw_clamp_adam_dev(L.dptr(b.flat), L.dptr(b.flat_grad), L.dptr(self.state["exp_avg"]),
                                             L.dptr(self.state["exp_avg_sq"]), L.BRAIN_NPARAMS, L.dptr(self.state["dev"]),
                                             g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], g["clamp"],
                                             self.grad_scale, L.stream_ptr(b.flat.device)), "clamp_adam_dev")

    def note_dev_steps(self, n=1):
        self.state["step"] += n
        self.state["dev_step"] = self.state["step"]

    def hyper(self):
        g = self.param_groups[0]
        return (self.kind, float(g["lr"]), tuple(g["betas"]), float(g["eps"]), float(g["weight_decay"]), float(g["clamp"])) + \
            self._schedule_hyper()

    def onecall_tail(self):
        g, s = self.param_groups[0], self.state
        if self.scheduled:
            return "ivosw_dqn_step_drawn_sched", (L.dptr(s["exp_avg"]), L.dptr(s["exp_avg_sq"]), L.dptr(s["dev"]), L.dptr(self.lr_table()),
                                                  self.schedule()[3], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], g["clamp"],
                                                  self.grad_scale)
        return "ivosw_dqn_step_drawn_ex", (L.dptr(s["exp_avg"]), L.dptr(s["exp_avg_sq"]), L.dptr(s["dev"]), g["lr"], g["betas"][0],
                                           g["betas"][1], g["eps"], g["weight_decay"], g["clamp"], self.grad_scale)

    def onecall_tgt_tail(self):
        """ivosw_dqn_step_drawn_tgt's arguments from `optimizer` to `grad_scale`."""
        g, s = self.param_groups[0], self.state
        table, n = (L.dptr(self.lr_table()), self.schedule()[3]) if self.scheduled else (None, 0)
        return (L.OPT_ADAM, L.dptr(s["exp_avg"]), L.dptr(s["exp_avg_sq"]), L.dptr(s["dev"]), g["lr"], table, n, g["betas"][0], g["betas"][1],
                g["eps"], 0.0, 0, g["weight_decay"], g["clamp"], self.grad_scale)

    def state_dict(self):
        self._ensure()
        return dict(state={k: (v.clone() if torch.is_tensor(v) else v) for k, v in self.state.items() if not k.startswith("dev")},
                    param_groups=[{k: v for k, v in self.param_groups[0].items() if k != "params"}])

    def load_state_dict(self, sd):
        self._ensure()
        self._load_schedule(sd)
        self.state["step"] = int(sd["state"]["step"])
        self.state["exp_avg"].copy_(sd["state"]["exp_avg"])
        self.state["exp_avg_sq"].copy_(sd["state"]["exp_avg_sq"])


class FusedClampSGD(_LrSchedule):
    """``optim.SGD(params, lr, momentum, dampening=0, weight_decay, nesterov)`` + the reference's grad clamp, as one kernel over the flat
    arena (ivosw_clamp_sgd).  The momentum buffer starts at zero, which makes torch's first step (buffer = d) the ordinary update, so
    nothing but the buffer carries over between steps: a captured step replays the update as it stands.  ``state["step"]`` only counts
    the updates on the host — except on the poly schedule, whose captured updates keep a step counter on the device too (``dev_state``;
    ivosw_clamp_sgd_dev_sched).  Same interface as FusedClampAdam."""

    kind = "sgd"

    def __init__(self, brain, lr, weight_decay, momentum=0.0, nesterov=False, clamp=1.0, lr_schedule="constant", lr_pow=None,
                 lr_total_steps=None):
        self.brain = brain
        self.param_groups = [dict(params=list(brain.parameters()), lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay,
                                  nesterov=nesterov, clamp=clamp)]
        self._init_schedule(lr_schedule, lr_pow, lr_total_steps)
        self.state = dict(step=0, momentum_buffer=None)
        self.grad_scale = 1.0

    def _ensure(self):
        flat = self.brain.flat
        if self.state["momentum_buffer"] is None or self.state["momentum_buffer"].device != flat.device:
            self.state["momentum_buffer"] = torch.zeros_like(flat)

    def zero_grad(self, set_to_none=False):
        self.brain.flat_grad.zero_()

    def step(self):
        self._ensure()
        lr = self.current_lr()
        self.state["step"] += 1
        self._clamp_sgd(lr)

    def _clamp_sgd(self, lr):
        g, b = self.param_groups[0], self.brain
        L.check(L.lib().ivosw_clamp_sgd(L.dptr(b.flat), L.dptr(b.flat_grad), L.dptr(self.state["momentum_buffer"]), L.BRAIN_NPARAMS, lr,
                                        g["momentum"], g["weight_decay"], int(g["nesterov"]), g["clamp"], self.grad_scale,
                                        L.stream_ptr(b.flat.device)), "clamp_sgd")

    def dev_state(self):
        """The device state of the update: the momentum buffer.  On the poly schedule also the 8-byte step counter on the device
        (``state["dev"]``), (re)synchronised with the host counter as FusedClampAdam's, and the schedule's table."""
        self._ensure()
        if self.scheduled:
            self.lr_table()
            dev = self.brain.flat.device
            ds = self.state.get("dev")
            if ds is None or ds.device != dev:
                ds = torch.zeros(L.lib().ivosw_sgd_state_bytes(), dtype=torch.uint8, device=dev)
                self.state["dev"], self.state["dev_step"] = ds, 0
            if self.state["dev_step"] != self.state["step"]:
                ds[0:4].copy_(torch.from_numpy(np.array([self.state["step"]], dtype=np.int32).view(np.uint8)))
                self.state["dev_step"] = self.state["step"]
        return self.state["momentum_buffer"]

    def enqueue_dev_step(self):
        """ivosw_clamp_sgd on the current stream (inside a capture: recorded as it is); on the poly schedule ivosw_clamp_sgd_dev_sched,
        which advances the device step counter."""
        if not self.scheduled:
            self._clamp_sgd(self.param_groups[0]["lr"])
            return
        g, b = self.param_groups[0], self.brain
        L.check(L.lib().ivosw_clamp_sgd_dev_sched(L.dptr(b.flat), L.dptr(b.flat_grad), L.dptr(self.state["momentum_buffer"]), L.BRAIN_NPARAMS,
                                                  L.dptr(self.state["dev"]), L.dptr(self.lr_table()), self.schedule()[3], g["momentum"],
                                                  g["weight_decay"], int(g["nesterov"]), g["clamp"], self.grad_scale,
                                                  L.stream_ptr(b.flat.device)), "clamp_sgd_dev_sched")

    def note_dev_steps(self, n=1):
        self.state["step"] += n
        if "dev" in self.state:
            self.state["dev_step"] = self.state["step"]

    def hyper(self):
        g = self.param_groups[0]
        return (self.kind, float(g["lr"]), float(g["momentum"]), bool(g["nesterov"]), float(g["weight_decay"]), float(g["clamp"])) + \
            self._schedule_hyper()

    def onecall_tail(self):
        g = self.param_groups[0]
        if self.scheduled:
            return "ivosw_dqn_step_drawn_sgd_sched", (L.dptr(self.state["momentum_buffer"]), L.dptr(self.state["dev"]), L.dptr(self.lr_table()),
                                                      self.schedule()[3], g["momentum"], g["weight_decay"], int(g["nesterov"]), g["clamp"],
                                                      self.grad_scale)
        return "ivosw_dqn_step_drawn_sgd", (L.dptr(self.state["momentum_buffer"]), g["lr"], g["momentum"], g["weight_decay"],
                                            int(g["nesterov"]), g["clamp"], self.grad_scale)

    def onecall_tgt_tail(self):
        """ivosw_dqn_step_drawn_tgt's arguments from `optimizer` to `grad_scale`."""
        g, s = self.param_groups[0], self.state
        table, n, dev = (L.dptr(self.lr_table()), self.schedule()[3], L.dptr(s["dev"])) if self.scheduled else (None, 0, None)
        return (L.OPT_SGD, L.dptr(s["momentum_buffer"]), None, dev, g["lr"], table, n, 0.0, 0.0, 0.0, g["momentum"], int(g["nesterov"]),
                g["weight_decay"], g["clamp"], self.grad_scale)

    def state_dict(self):
        self._ensure()
        return dict(state=dict(step=self.state["step"], momentum_buffer=self.state["momentum_buffer"].clone()),
                    param_groups=[{k: v for k, v in self.param_groups[0].items() if k != "params"}])

    def load_state_dict(self, sd):
        st = sd["state"]
        if "momentum_buffer" not in st or "exp_avg" in st:
            raise ValueError("FusedClampSGD.load_state_dict: not an SGD state dict (an Adam one has exp_avg / exp_avg_sq)")
        self._ensure()
        self._load_schedule(sd)
        self.state["step"] = int(st["step"])
        self.state["momentum_buffer"].copy_(st["momentum_buffer"])


def candidates_option(candidates=1, skip_annotated=False):
    """(k, skip), checked: cfg.agent.candidates an int in [1, L.MAX_CANDIDATES] and cfg.agent.skip_annotated a bool.  Anything else is a
    ValueError that names the key."""
    if isinstance(candidates, bool) or not isinstance(candidates, int) or not 1 <= candidates <= L.MAX_CANDIDATES:
        raise ValueError(f"agent.candidates must be an int in [1, {L.MAX_CANDIDATES}], got {candidates!r}")
    if not isinstance(skip_annotated, bool):
        raise ValueError(f"agent.skip_annotated must be true or false, got {skip_annotated!r}")
    return candidates, skip_annotated


MAX_CANDIDATE_GAP = 1 << 20                 # RAGGED_MAX_ROWS: a larger distance than any sequence is long says nothing more


def candidate_gap_option(candidate_gap=1):
    """gap, checked: cfg.agent.candidate_gap an int in [1, 2^20] (1: the plain ranking).  Anything else, a bool included, is a ValueError
    that names the key."""
    if isinstance(candidate_gap, bool) or not isinstance(candidate_gap, int) or not 1 <= candidate_gap <= MAX_CANDIDATE_GAP:
        raise ValueError(f"agent.candidate_gap must be an int in [1, {MAX_CANDIDATE_GAP}], got {candidate_gap!r}")
    return candidate_gap


def spread_candidates(ranking):
    """The candidate list of one state from a ranking that ivosw_brain_topk_spread_ragged wrote (the forced first candidate already in
    slot 0, every slot at least the gap from the others): its -1 slots cut off, as a host np.int64 array.  Nothing is spliced in."""
    rank = np.asarray(ranking, dtype=np.int64).reshape(-1)
    return rank[rank >= 0]


def merge_candidates(pick, ranking, k):
    """The candidate list of one state as a host np.int64 array: the device ranking (its -1 slots cut off), cut to k.  With a random
    pick of the epsilon branch (``pick`` not None) the pick comes first and the ranking follows with that frame removed."""
    rank = np.asarray(ranking, dtype=np.int64).reshape(-1)
    rank = rank[rank >= 0]
    if pick is not None:
        rank = np.concatenate([np.array([int(pick)], dtype=np.int64), rank[rank != int(pick)]])
    return rank[:k]


class Agent(nn.Module):
    def __init__(self, device, cfg):
        super().__init__()
        self.cfg = cfg
        self.device = device
        a = cfg.agent
        self.memory_size = a.memory_size
        self.GAMMA = a.gamma
        self.loss_kind, self.huber_delta = self._loss_option(a)
        self.lr_schedule, self.lr_pow, self.lr_total_steps = self._lr_schedule_option(a)
        self.replay_kind, self.per_alpha, self.per_beta, self.per_beta_steps, self.per_eps = self._replay_option(a)
        self.per_replay = None                      # the PrioritizedReplay of the episode loop (utils_agent._device_update_loop)
        self.target_update, self.tau, self.target_period = self._target_option(a)
        self.candidates, self.skip_annotated = self._candidates_option(a)
        self.candidate_gap = self._candidate_gap_option(a)
        self.target_steps = 0                       # steps the device rule has seen (soft / periodic); resumed by load_target_state
        self._target_dev, self._target_dev_step = None, 0
        self.EPS_START, self.EPS_END, self.EPS_DECAY = a.eps_start, a.eps_end, a.eps_decay
        self.steps_done = 0
        self.update_rate = a.update_rate
        self.subset = cfg.data.subset
        self.memory_pool = ReplayMemory(self.memory_size)

        self.policy_net = Brain()
        self.target_net = Brain()
        self.target_net.load_state_dict(self.policy_net.state_dict())
        self.policy_net.to(self.device)
        self.target_net.to(self.device)

        self.loss = []
        self.loss_position = 0
        self.loss_capacity = 32
        self.loss_avg = 0
        self.optimizer_kind, self.momentum, self.nesterov = self._optimizer_option(a)
        sched = dict(lr_schedule=self.lr_schedule, lr_pow=self.lr_pow, lr_total_steps=self.lr_total_steps)
        if self.optimizer_kind == "sgd":
            self.optimizer = FusedClampSGD(self.policy_net, lr=a.lr, weight_decay=a.weight_decay, momentum=self.momentum,
                                           nesterov=self.nesterov, **sched)
        else:
            self.optimizer = FusedClampAdam(self.policy_net, lr=a.lr, weight_decay=a.weight_decay, **sched)
        self._ws = L.Workspace()
        self._loss_dev = None

    @staticmethod
    def _loss_option(a):
        """cfg.agent.loss ("mse", the reference's two-term MSE and the default; or "huber") and cfg.agent.huber_delta (1.0, torch's
        default): read with .get, so a config without the keys trains with MSE as before; anything else is refused."""
        kind = a.get("loss", "mse")
        if kind not in ("mse", "huber"):
            raise ValueError(f"agent.loss must be 'mse' or 'huber', got {kind!r}")
        delta = a.get("huber_delta", 1.0)
        if isinstance(delta, bool) or not isinstance(delta, (int, float)) or not 0 < delta <= float(np.finfo(np.float32).max):
            raise ValueError(f"agent.huber_delta must be a finite number > 0, got {delta!r}")
        return kind, float(delta)

    _LOSS_KINDS = {"mse": L.DQN_LOSS_MSE, "huber": L.DQN_LOSS_HUBER}

    @staticmethod
    def _optimizer_option(a):
        """cfg.agent.optimizer ("adam", the reference's and the default; or "sgd"), cfg.agent.momentum (0.0, torch's default; the CLI and
        YAML defaults give 0.9) and cfg.agent.nesterov (False): read with .get, so a config without the keys trains with Adam as before,
        which ignores momentum and nesterov; anything else is refused."""
        kind = a.get("optimizer", "adam")
        if kind not in ("adam", "sgd"):
            raise ValueError(f"agent.optimizer must be 'adam' or 'sgd', got {kind!r}")
        momentum = a.get("momentum", 0.0)
        if isinstance(momentum, bool) or not isinstance(momentum, (int, float)) or not 0 <= momentum <= float(np.finfo(np.float32).max):
            raise ValueError(f"agent.momentum must be a finite number >= 0, got {momentum!r}")
        nesterov = a.get("nesterov", False)
        if not isinstance(nesterov, bool):
            raise ValueError(f"agent.nesterov must be true or false, got {nesterov!r}")
        if kind == "sgd" and nesterov and momentum == 0:
            raise ValueError("agent.nesterov needs agent.momentum > 0 (as torch.optim.SGD)")
        return kind, float(momentum), nesterov

    @staticmethod
    def _lr_schedule_option(a):
        """cfg.agent.lr_schedule ("constant", the reference's fixed lr and the default; or "poly"), cfg.agent.lr_pow (0.9, the reference's
        config) and cfg.agent.lr_total_steps (N, required by "poly"; 0 = unset): read with .get, so a config without the keys keeps the
        constant lr; lr_pow and N are only checked under "poly".  Returns (schedule, lr_pow, N), (schedule, None, None) for "constant";
        anything else is refused (lr_schedule_option), before anything is allocated."""
        return lr_schedule_option(a.get("lr_schedule", "constant"), a.get("lr_pow", 0.9), a.get("lr_total_steps", 0))

    @staticmethod
    def _replay_option(a):
        """cfg.agent.replay ("uniform", today's minibatches and the default; or "prioritized") and the PER keys per_alpha (0.6), per_beta
        (beta0, 0.4), per_beta_steps (0: beta stays beta0) and per_eps (1e-6): read with .get, so a config without them trains as before;
        checked by replay_option, before anything is allocated."""
        return replay_option(a.get("replay", "uniform"), a.get("per_alpha", 0.6), a.get("per_beta", 0.4), a.get("per_beta_steps", 0),
                             a.get("per_eps", 1e-6))

    @staticmethod
    def _target_option(a):
        """cfg.agent.target_update ("coin", the reference's hard sync with probability update_rate and the default; "soft": Polyak
        averaging with cfg.agent.tau (0.005) after every step; "periodic": a hard sync every cfg.agent.target_period-th (20) step): read
        with .get, so a config without the keys keeps the coin; tau and target_period are only checked under their mode
        (target_update_option), before anything is allocated.  update_rate is only read under "coin"."""
        return target_update_option(a.get("target_update", "coin"), a.get("tau", 0.005), a.get("target_period", 20))

    @staticmethod
    def _candidates_option(a):
        """cfg.agent.candidates (1, the reference's single frame and the default: how many ranked frames action / actions return per
        state) and cfg.agent.skip_annotated (False: frames that were annotated before rank behind all others, select_next_frame's rule):
        read with .get, so a config without the keys acts as before; checked by candidates_option, before anything is allocated."""
        return candidates_option(a.get("candidates", 1), a.get("skip_annotated", False))

    @staticmethod
    def _candidate_gap_option(a):
        """cfg.agent.candidate_gap (1, the plain ranking and the default: the least distance in frames between any two of the k candidates
        of a state, ivosw_brain_topk_spread_ragged's greedy rule): read with .get, so a config without the key acts as before; checked
        by candidate_gap_option, before anything is allocated.  Without effect at candidates = 1."""
        return candidate_gap_option(a.get("candidate_gap", 1))

    def _spread_gap(self, k):
        """The gap the device ranking of k candidates runs under: 1 (the plain ranking, today's calls) unless k > 1 and a gap is set."""
        gap = candidate_gap_option(getattr(self, "candidate_gap", 1))
        return gap if k > 1 else 1

    def prioritized_replay(self, soa, device, seed):
        """A PrioritizedReplay over `soa` with this agent's PER options."""
        if self.replay_kind != "prioritized":
            raise ValueError("agent.replay is not 'prioritized'")
        return PrioritizedReplay(soa, device, self.per_alpha, self.per_beta, self.per_beta_steps, self.per_eps, seed=seed)

    def _loss_args(self):
        """(loss_kind, huber_delta) as the _ex entries take them (IVOSW_DQN_LOSS_*, fp32)."""
        if self.loss_kind not in self._LOSS_KINDS:
            raise ValueError(f"agent.loss_kind must be 'mse' or 'huber', got {self.loss_kind!r}")
        return self._LOSS_KINDS[self.loss_kind], float(np.float32(self.huber_delta))

    # ------------------------------------------------------------------ data-parallel hook
    @staticmethod
    def _world():
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist, dist.get_world_size()
        return None, 1

    # ------------------------------------------------------------------ DQN update
    def _device_batch(self, sample):
        """Collated DataLoader dict (datasets/agent_dataset.py) or a DeviceReplay.sample() dict -> device tensors."""
        dev = self.device
        if "state" in sample:                       # already gathered on device (ivosw_replay_gather)
            return (sample["state"], sample["new_state"], sample["action"], sample["reward_step"],
                    sample["reward_done"])
        B = sample["action"].shape[0]
        col = lambda k: torch.as_tensor(sample[k]).reshape(B, -1).to(torch.float32)
        state = torch.stack([col("old_state_iou"), col("annotated_frames")], 2).contiguous().to(dev)
        new_state = torch.stack([col("new_state_iou"), col("next_annotated_frames")], 2).contiguous().to(dev)
        action = torch.as_tensor(sample["action"]).reshape(B).to(torch.int64).to(dev)
        r_step = torch.as_tensor(sample["reward_step"]).reshape(B).to(torch.float32).to(dev)
        r_done = torch.as_tensor(sample["reward_done"]).reshape(B).to(torch.float32).to(dev)
        return state, new_state, action, r_step, r_done       # 'done' is loaded but unused upstream (agent.py:114)

    def loss_and_grads(self, sample):
        """Forward x3 + loss + backward into policy_net.flat_grad (unclamped). Returns the device loss scalar.  A sample that carries
        ``weights`` (PrioritizedReplay.sample_prioritized) takes the importance-weighted loss (ivosw_dqn_loss_grad_per), and the rows' TD
        errors |e1| + |e2| stay on the device in ``sample["td"]`` (or ``self.last_td``) for update_priorities."""
        state, new_state, action, r_step, r_done = self._device_batch(sample)
        B, T, _ = state.shape
        lib = L.lib()
        nbytes = lib.ivosw_dqn_ws_bytes(B, T)
        ws = self._ws.get(nbytes, state.device)
        if self._loss_dev is None or self._loss_dev.device != state.device:
            self._loss_dev = torch.zeros(1, dtype=torch.float32, device=state.device)
        pn, tn = self.policy_net, self.target_net
        if "weights" in sample:
            td = sample.get("td")
            if td is None:
                td = torch.empty(B, dtype=torch.float32, device=state.device)
            self.last_td = td
            L.check(lib.ivosw_dqn_loss_grad_per(L.dptr(pn.flat), L.dptr(tn.flat), L.dptr(state), L.dptr(new_state),
                                                L.dptr(action, torch.int64), L.dptr(r_step), L.dptr(r_done), B, T,
                                                float(np.float32(self.GAMMA)), *self._loss_args(), L.dptr(sample["weights"]), L.dptr(td),
                                                L.dptr(pn.flat_grad), L.dptr(self._loss_dev), L.dptr(ws), nbytes, L.stream_ptr(state.device)),
                    "dqn_loss_grad_per")
            return self._loss_dev
        L.check(lib.ivosw_dqn_loss_grad_ex(L.dptr(pn.flat), L.dptr(tn.flat), L.dptr(state), L.dptr(new_state),
                                           L.dptr(action, torch.int64), L.dptr(r_step), L.dptr(r_done), B, T,
                                           float(np.float32(self.GAMMA)), *self._loss_args(), L.dptr(pn.flat_grad),
                                           L.dptr(self._loss_dev), L.dptr(ws), nbytes, L.stream_ptr(state.device)), "dqn_loss_grad")
        return self._loss_dev

    def update_agent(self, sample):
        """The reference's update on one collated batch.  It stays unweighted under agent.replay = "prioritized": an explicit batch has no
        draw probabilities; the prioritized episode loop is utils_agent._device_update_loop."""
        if sample is None:
            print("no input")
            return
        loss = self.loss_and_grads(sample)
        self._update_avg_loss(loss)                 # synchronises (loss.item(), models/agent.py:166): the P2P error word rides with it
        self.apply_gradients()
        if self.target_step():
            print("target_net updated!")
        return self.loss[(self.loss_position - 1) % self.loss_capacity]

    def apply_gradients(self, check_every=1):
        """clamp + Adam (or clamp + SGD) on policy_net.flat_grad; with torch.distributed initialised: synchronous data parallel — the
        gradients are summed over the ranks first (RCCL over xGMI, or the opt-in one-shot P2P all-reduce fused with the update) and
        averaged inside the kernel, so the clamp sees the averaged gradient as a single large batch would."""
        dist, world = self._world()
        if world > 1 or dist is not None:           # an initialised process group of one rank (IVOSW_FORCE_DIST=1) takes the same path
            from .. import parallel
            parallel.data_parallel_step(self.policy_net, self.optimizer, check_every)
        else:
            self.optimizer.step()

    def sync_target(self):
        pn, tn = self.policy_net, self.target_net
        L.check(L.lib().ivosw_copy_f32(L.dptr(tn.flat), L.dptr(pn.flat), L.BRAIN_NPARAMS,
                                       L.stream_ptr(pn.flat.device)), "copy_f32")

    # ------------------------------------------------------------------ target-network rule
    def target_step(self):
        """The target rule after one policy update, where the reference flips its coin.  "coin": one np.random draw, a hard sync
        (sync_target) with probability update_rate; np.random is seeded identically on every rank.  "soft" / "periodic": no random number
        is drawn - ivosw_target_update is enqueued, a pure function of device state, the same on every rank.  Returns whether the target
        was hard-synced."""
        if self.target_update == "coin":
            if np.random.random() < self.update_rate:
                self.sync_target()
                return True
            return False
        self.target_dev_state()
        self.enqueue_target_update()
        return self.note_target_steps(1) > 0

    def target_hyper(self):
        """(target_update, tau, period) as the attributes hold them now (checked): what a captured step bakes in."""
        return target_update_option(self.target_update, self.tau, self.target_period)

    def target_dev_state(self):
        """The 16-byte state of the device rule (the step counter at byte 0), created on first use and (re)synchronised with
        ``target_steps``."""
        dev = self.policy_net.flat.device
        ds = self._target_dev
        if ds is None or ds.device != dev:
            ds = self._target_dev = torch.zeros(L.lib().ivosw_target_state_bytes(), dtype=torch.uint8, device=dev)
            self._target_dev_step = 0
        if self._target_dev_step != self.target_steps:
            ds[0:4].copy_(torch.from_numpy(np.array([self.target_steps], dtype=np.int32).view(np.uint8)))
            self._target_dev_step = self.target_steps
        return ds

    def _target_args(self):
        """(mode, tau, period) as the C entries take them (IVOSW_TARGET_*, fp32 tau)."""
        kind, tau, period = self.target_hyper()
        if kind == "coin":
            raise ValueError("agent.target_update = 'coin' has no device rule (Agent.target_step flips the coin)")
        return _TARGET_MODES[kind], float(np.float32(tau)) if tau is not None else 0.0, period if period is not None else 1

    def enqueue_target_update(self):
        """ivosw_target_update on the current stream (inside a capture: recorded); the caller has called target_dev_state and bumps the
        host counter per replay (note_target_steps)."""
        pn, tn = self.policy_net, self.target_net
        L.check(L.lib().ivosw_target_update(L.dptr(tn.flat), L.dptr(pn.flat), L.BRAIN_NPARAMS, *self._target_args(),
                                            L.dptr(self._target_dev), L.stream_ptr(pn.flat.device)), "target_update")

    def note_target_steps(self, n=1):
        """The host counter after n device steps of the rule; returns how many of them hard-synced the target (0 under soft)."""
        before = self.target_steps
        self.target_steps += n
        self._target_dev_step = self.target_steps
        if self.target_update != "periodic":
            return 0
        return self.target_steps // self.target_period - before // self.target_period

    def target_state(self):
        """What a resume restores of the target rule besides the two networks: the mode and the step counter."""
        return dict(target_update=self.target_update, target_steps=int(self.target_steps))

    def load_target_state(self, sd):
        if sd.get("target_update", self.target_update) != self.target_update:
            raise ValueError(f"the saved target state is for target_update {sd['target_update']!r}, this agent runs {self.target_update!r}")
        self.target_steps = int(sd["target_steps"])          # the device counter follows at the next step (target_dev_state)

    # ------------------------------------------------------------------ acting
    def action(self, state, verbose=True, device_out=None):
        """Reference surface: action(state [T,2] numpy, verbose) -> frame index (agent.py:168-196).  Extensions used by
        utils_agent's device-resident chain: `state` may be a [T,2] fp32 CUDA tensor, and with `device_out` (int64 [1] on
        the device) the greedy index is left THERE and None is returned, so the caller can fetch it together with its
        other results in one D2H copy (the epsilon branch still returns a host integer).

        With agent.skip_annotated the greedy index is slot 0 of the masked ranking (``candidates_device``): same types, same host work.
        With agent.candidates = k > 1 the return is an np.int64 array of min(k, T) frames: the ranking on the greedy branch; on the epsilon
        branch the random pick, then the ranking with that frame removed (``merge_candidates``).  `device_out` is then int64 [k]: the
        ranking is left there on either branch and the caller merges (None, or the random pick, is returned).

        With agent.candidate_gap = g > 1 (and k > 1) the candidates are at least g frames apart (ivosw_brain_topk_spread_ragged): the random
        pick goes to the device as the forced first candidate, so the ranking that comes back is the candidate list as it stands (its -1
        slots cut off: it may be shorter than k) and nothing is merged, by this method or, with `device_out`, by the caller."""
        pick = self._host_pick(state, verbose)
        k, skip = candidates_option(self.candidates, self.skip_annotated)
        if pick is not None and k == 1:
            return pick
        on_device = torch.is_tensor(state) and state.is_cuda       # [T,2] fp32 already on the GPU (utils_agent's device chain)
        st = state if on_device else torch.as_tensor(np.asarray(state), dtype=torch.float32).to(self.device)
        if k == 1 and not skip:
            if device_out is not None:
                self.greedy_index_device(st, out=device_out)
                return None
            return np.int64(self.greedy_index_device(st).item())
        gap = self._spread_gap(k)
        if gap > 1:
            rank = self.candidates_device([st], k, skip, out=device_out, gap=gap, first=[-1 if pick is None else int(pick)])
            return pick if device_out is not None else spread_candidates(rank.cpu().numpy()[0])
        rank = self.candidates_device([st], k, skip, out=device_out)
        if device_out is not None:
            return pick
        host = rank.cpu().numpy()
        return np.int64(host[0, 0]) if k == 1 else merge_candidates(pick, host[0], k)

    def _host_pick(self, state, verbose):
        """The host half of one action (agent.py:168-185): steps_done, the epsilon threshold, the random.random() draw and the log line;
        on the random branch the random.choice pick, on the greedy branch None."""
        self.steps_done += 1
        if self.cfg.phase != "train":
            eps_threshold = 0
        else:
            eps_threshold = self.EPS_END + (self.EPS_START - self.EPS_END) * \
                math.exp(-0.5 * self.steps_done / self.EPS_DECAY)
        on_device = torch.is_tensor(state) and state.is_cuda
        n_frames = state.shape[0] if on_device else np.asarray(state).shape[0]
        rand_flag = random.random()
        greedy = rand_flag > eps_threshold
        if verbose:
            print(f"step:{self.steps_done}, rand_flag:{rand_flag:.4f}, eps_threshold:{eps_threshold:.4f}, "
                  f"frame index was selected {'by agent' if greedy else 'randomly'}")
        return None if greedy else random.choice(np.array(range(n_frames)))

    def actions(self, states, verbose=True, device_out=None):
        """``action`` for several states: per state, in order, exactly the host work of ``action`` (steps_done, the epsilon threshold,
        random.random(), the log line, random.choice on the random branch), then ONE ragged forward + ONE ragged argmax over all states
        (``greedy_indices_device``).  Returns a list with one entry per state: the host integer of a random pick, otherwise the greedy
        index - or None when ``device_out`` (int64 [K] on the device) is given: entry k of it then holds state k's greedy index (also
        for random-branch states, whose entry the caller ignores).  The host RNG streams and ``steps_done`` end where K sequential
        ``action`` calls leave them.

        With agent.skip_annotated / agent.candidates = k the argmax is the ragged masked top-k (``candidates_device``) and the entries are
        what ``action`` returns in that mode; ``device_out`` is int64 [K, k] and holds every state's ranking.  With agent.candidate_gap > 1
        the random picks are the forced first candidates of that ranking, which is then final (see ``action``)."""
        states = list(states)
        picks = [self._host_pick(state, verbose) for state in states]
        k, skip = candidates_option(self.candidates, self.skip_annotated)
        if not states or (k == 1 and all(p is not None for p in picks)):      # nothing is greedy: no forward, as under `action`
            return picks
        if k == 1 and not skip:
            idx = self.greedy_indices_device(states, out=device_out)
            if device_out is not None:
                return picks
            host = idx.cpu().numpy()
            return [p if p is not None else np.int64(host[i]) for i, p in enumerate(picks)]
        gap = self._spread_gap(k)
        if gap > 1:
            rank = self.candidates_device(states, k, skip, out=device_out, gap=gap, first=[-1 if p is None else int(p) for p in picks])
            if device_out is not None:
                return picks
            host = rank.cpu().numpy()
            return [spread_candidates(host[i]) for i in range(len(states))]
        rank = self.candidates_device(states, k, skip, out=device_out)
        if device_out is not None:
            return picks
        host = rank.cpu().numpy()
        if k == 1:
            return [p if p is not None else np.int64(host[i, 0]) for i, p in enumerate(picks)]
        return [merge_candidates(p, host[i], k) for i, p in enumerate(picks)]

    def candidates_device(self, states, k=None, skip_annotated=None, out=None, gap=1, first=None):
        """The k strongest frames of every state ([T_k,2]; host arrays are uploaded) by Q, annotated frames last under skip_annotated
        (ivosw_brain_topk_ragged's order), left on the device: int64 [K, k] (or written to `out`, K k int64 values), -1 behind a state's
        last frame.  k and skip_annotated default to the agent's options.  One Brain.forward_ragged and one top-k launch per 128 states;
        a single state runs Brain.forward and the same entry with one sequence.  `gap` > 1 / `first` (one forced first candidate per
        state, -1 for none): ``topk_ragged``'s spread ranking."""
        k, skip = candidates_option(self.candidates if k is None else k, self.skip_annotated if skip_annotated is None else skip_annotated)
        dev = self.policy_net.flat.device
        sts = [s if (torch.is_tensor(s) and s.is_cuda) else torch.as_tensor(np.asarray(s), dtype=torch.float32).to(dev) for s in states]
        if not sts:
            raise ValueError("candidates_device needs at least one state")
        lengths = [int(s.shape[0]) for s in sts]
        if len(sts) == 1:
            x = sts[0].detach().to(dtype=torch.float32).contiguous()
            q = self.policy_net(x[None]).view(-1)
        else:
            x = _adjacent_rows(sts)                           # slices of one flat [R,2] tensor, in order: read in place
            if x is None:
                x = torch.cat([s.detach().to(dtype=torch.float32) for s in sts], 0)
            x = x.detach().to(dtype=torch.float32).contiguous()
            q, _ = self.policy_net.forward_ragged(x, lengths)
        if gap == 1 and first is None:
            return self.topk_ragged(q, x, lengths, k, skip, out=out)
        return self.topk_ragged(q, x, lengths, k, skip, out=out, gap=gap, first=first)

    def topk_ragged(self, q, states, lengths, k, skip, out=None, qv=None, gap=1, first=None):
        """ivosw_brain_topk_ragged over the flat q [R] of sequences of `lengths`: int64 [K, k] on the device (or `out`), the j-th
        strongest frame of every sequence, -1 from its length on.  `states` is the flat [R,2] fp32 state whose column 1 holds the
        annotation counts, or None (only with `skip` false); `qv` (float32 [K, k], optional) receives the Q values of the slots.

        With `gap` > 1 or `first` (K host ints: the forced first candidate of every sequence, -1 for none) the entry is
        ivosw_brain_topk_spread_ragged: the same order walked greedily, a frame accepted only `gap` or more frames from every accepted one,
        -1 from the slot on at which nothing more can be accepted."""
        K = len(lengths)
        idx = out.view(K, k) if out is not None else torch.empty(K, k, dtype=torch.int64, device=q.device)
        if qv is not None:
            qv = qv.view(K, k)
        spread = gap != 1 or first is not None
        if first is not None and len(first) != K:
            raise ValueError(f"topk_ragged: {len(first)} forced first candidates for {K} sequences")
        lib, off = L.lib(), 0
        for g in range(0, K, L.MAX_SEQS):
            group = lengths[g:g + L.MAX_SEQS]
            rows = sum(group)
            head = (L.dptr(q[off:off + rows], torch.float32), L.dptr(states[off:off + rows], torch.float32) if states is not None else None,
                    L.int_array(group), len(group), int(k), int(bool(skip)))
            tail = (L.dptr(idx[g:g + len(group)], torch.int64), L.dptr(qv[g:g + len(group)], torch.float32) if qv is not None else None,
                    L.stream_ptr(q.device))
            if spread:
                L.check(lib.ivosw_brain_topk_spread_ragged(*head, int(gap), L.int_array(first[g:g + len(group)]) if first is not None else None,
                                                           *tail), "topk_spread_ragged")
            else:
                L.check(lib.ivosw_brain_topk_ragged(*head, *tail), "topk_ragged")
            off += rows
        return idx

    def greedy_indices_device(self, states, out=None):
        """argmax_t Q(state_k)[t] for several states ([T_k,2]; host arrays are uploaded), left on the device (int64 [K], or written to
        `out`): one Brain.forward_ragged and one ivosw_brain_argmax_ragged per 128 states."""
        dev = self.policy_net.flat.device
        sts = [s if (torch.is_tensor(s) and s.is_cuda) else torch.as_tensor(np.asarray(s), dtype=torch.float32).to(dev) for s in states]
        lengths = [int(s.shape[0]) for s in sts]
        q, _ = self.policy_net.forward_ragged(sts)
        return self.argmax_ragged(q, lengths, out=out)

    def argmax_ragged(self, q, lengths, out=None):
        """The first maximum of every sequence's slice of the flat q -> int64 [K] on the device (or `out`)."""
        idx = out if out is not None else torch.empty(len(lengths), dtype=torch.int64, device=q.device)
        lib, off = L.lib(), 0
        for g in range(0, len(lengths), L.MAX_SEQS):
            group = lengths[g:g + L.MAX_SEQS]
            rows = sum(group)
            L.check(lib.ivosw_brain_argmax_ragged(L.dptr(q[off:off + rows]), L.int_array(group), len(group), L.dptr(idx[g:g + len(group)]),
                                                  L.stream_ptr(q.device)), "argmax_ragged")
            off += rows
        return idx

    def greedy_index_device(self, state, out=None):
        """argmax_t Q(state)[t] for a device state [T,2] fp32, result left on the device (int64 [1], or written to `out`)."""
        q = self.policy_net(state[None])
        idx = out if out is not None else torch.empty(1, dtype=torch.int64, device=q.device)
        L.check(L.lib().ivosw_brain_argmax(L.dptr(q), 1, q.shape[1], L.dptr(idx), L.stream_ptr(q.device)), "argmax")
        return idx

    # ------------------------------------------------------------------ bookkeeping
    def _update_avg_loss(self, loss):
        self.note_loss(float(loss.detach().to("cpu").reshape(-1)[0]))

    def note_loss(self, value):
        """The 32-entry loss ring of the reference (models/agent.py:198-203), fed with a host float."""
        if len(self.loss) < self.loss_capacity:
            self.loss.append(None)
        self.loss[self.loss_position] = float(value)
        self.loss_position = (self.loss_position + 1) % self.loss_capacity
        self.loss_avg = sum(self.loss) / len(self.loss)

    def get_avg_loss(self):
        return self.loss_avg

    def set_train(self):
        self.policy_net.train()
        self.target_net.train()

    def set_eval(self):
        self.policy_net.eval()
        self.target_net.eval()

    def memory(self, state, old_frame, next_state, reward_step, reward_done, is_done, state_iou, next_state_iou,
               annotated_frames_str, next_annotated_frames_str, report_save_dir):
        self.memory_pool.push(state, old_frame, next_state, reward_step, reward_done, is_done, state_iou,
                              next_state_iou, annotated_frames_str, next_annotated_frames_str)
        self.memory_pool.push_to_csv(report_save_dir)


class CapturedDqnStep:
    """One Double-DQN training step as ONE HIP-graph launch (models/agent.py:128-160 minus the host coin flip):

        replay gather (minibatch indices read from ``self.idx`` on the device) -> 3 forwards + loss + BPTT
        -> [fused=True: the update — clamp + Adam with the step counter on the device, or clamp + SGD
            -> under agent.target_update = "soft" / "periodic" the target rule: in the update's own launch on the one-call chain,
               ivosw_target_update elsewhere.  Under "coin" the caller flips the coin (Agent.target_step) after the launch.]

    With fused=False the graph stops at the gradients, for the data-parallel step (all-reduce, then the eager update, then
    Agent.target_step in every mode).
    Replaces ~40 host launches (170-250 us of enqueue per step) by one hipGraphLaunch.  The arithmetic is the eager path's:
    the same entry points are recorded, so results are bit-identical to ``Agent.loss_and_grads`` + ``optimizer.step``."""

    def __init__(self, agent, replay, B, fused=True, draw_seed=None, steps=1, draw_state=None, capture=True):
        """draw_seed: None = the caller writes the minibatch rows into ``self.idx`` before every launch; an integer = the rows
        are drawn INSIDE the graph (``ivosw_replay_draw_gather``, uniform with replacement from a device-side counter-based
        generator seeded with it), ``self.idx`` then holds the rows of the last launch.  draw_state: share another captured
        step's generator state instead of creating one.  steps > 1 (needs the in-graph draw and fused=True): that many
        consecutive training steps per launch — everything a step changes (parameters, Adam moments and step counter, draw
        counter, the target rule's counter) lives on the device, so the recorded sequence simply repeats; under
        agent.target_update = "coin" the caller owns the host-side coin of the target sync, i.e. launches a multi-step graph only over
        steps whose coins do not fire (``GraphedDqnLoop``)."""
        dev = torch.device(agent.device)
        self.agent, self.replay, self.B, self.fused, self.steps = agent, replay, B, fused, int(steps)
        # a PrioritizedReplay: the step is the composed chain draw + gather (ivosw_per_draw_gather) -> weighted loss and gradients
        # (ivosw_dqn_loss_grad_per) -> the optimizer's device update -> priority update (ivosw_per_update); the draw state is the replay's
        self.per = isinstance(replay, PrioritizedReplay)
        if self.per:
            if not fused:
                raise ValueError("a prioritized step needs the fused update (agent.replay = 'prioritized' has no data-parallel form)")
            if draw_state is not None and draw_state is not replay.state:
                raise ValueError("a prioritized step draws with its replay's own state (PrioritizedReplay.state)")
            if draw_seed is not None and (int(draw_seed) & 0xFFFF_FFFF_FFFF_FFFF) != replay.seed:
                raise ValueError(f"a prioritized step draws with its replay's seed ({replay.seed}), not {draw_seed}")
            self.draw = replay.state
            self.weights = torch.empty(B, dtype=torch.float32, device=dev)
            self.td = torch.zeros(B, dtype=torch.float32, device=dev)
        else:
            self.draw = draw_state if draw_state is not None else (replay.draw_state(draw_seed) if draw_seed is not None else None)
        if self.steps > 1 and (self.draw is None or not fused):
            raise ValueError("a multi-step graph needs the in-graph minibatch draw and the fused update")
        T = replay.T
        lib = L.lib()
        self.idx = torch.zeros(B, dtype=torch.int64, device=dev)
        self.state = torch.empty(B, T, 2, dtype=torch.float32, device=dev)
        self.new_state = torch.empty_like(self.state)
        self.action = torch.empty(B, dtype=torch.int64, device=dev)
        self.r_step = torch.empty(B, dtype=torch.float32, device=dev)
        self.r_done = torch.empty_like(self.r_step)
        self.loss = torch.zeros(1, dtype=torch.float32, device=dev)
        nbytes = lib.ivosw_dqn_ws_bytes(B, T)
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        pn, tn, opt = agent.policy_net, agent.target_net, agent.optimizer
        self.tgt = fused and agent.target_hyper()[0] != "coin"          # the target rule is part of the step
        if fused:
            opt.dev_state()
        if self.tgt:
            agent.target_dev_state()
        self._keys = (pn.flat.data_ptr(), tn.flat.data_ptr(), pn.flat_grad.data_ptr())
        self._hyper = self._hyper_now()          # the optimizer's kind and values / grad_scale / gamma / loss option are baked in
        self._nbytes, self.graph, self.kernel_nodes, self._onecall_args, self._onecall_entry = nbytes, None, None, None, None
        if not capture:                          # capture=False: the same launches, enqueued plainly by launch() (LeanDqnLoop)
            return
        torch.cuda.synchronize(dev)
        with L.Graph.capture(dev) as g:
            self._enqueue()
        self.graph = g
        self.kernel_nodes = g.kernel_nodes

    def _enqueue(self):
        """The step's launches on the current stream (recorded when a capture is open)."""
        agent, replay, B, fused = self.agent, self.replay, self.B, self.fused
        dev = torch.device(agent.device)
        lib, T, nbytes = L.lib(), replay.T, self._nbytes
        pn, tn, opt = agent.policy_net, agent.target_net, agent.optimizer
        for _ in range(self.steps):
            st = L.stream_ptr(dev)
            r = replay
            if self.per:
                batch = r.sample_prioritized(B, out=dict(idx=self.idx, weights=self.weights, td=self.td, state=self.state,
                                                         new_state=self.new_state, action=self.action, reward_step=self.r_step,
                                                         reward_done=self.r_done))
                L.check(lib.ivosw_dqn_loss_grad_per(L.dptr(pn.flat), L.dptr(tn.flat), L.dptr(self.state), L.dptr(self.new_state),
                                                    L.dptr(self.action), L.dptr(self.r_step), L.dptr(self.r_done), B, T,
                                                    float(np.float32(agent.GAMMA)), *agent._loss_args(), L.dptr(batch["weights"]),
                                                    L.dptr(self.td), L.dptr(pn.flat_grad), L.dptr(self.loss), L.dptr(self.ws), nbytes, st),
                        "dqn_loss_grad_per")
                opt.enqueue_dev_step()
                r.update_priorities(self.idx, self.td)
                if self.tgt:
                    agent.enqueue_target_update()
                continue
            if self.draw is not None and fused:
                # draw + gather folded into the encoder launch, the slab reduction into the update: 8 kernel nodes per step instead of 10
                if self._onecall_args is None:   # every pointer and scalar is fixed for the life of the object (launch() checks): built once
                    if self.tgt:                 # the rule rides in the update's launch: still 8 kernel nodes
                        self._onecall_entry = "ivosw_dqn_step_drawn_tgt"
                        tail = opt.onecall_tgt_tail() + agent._target_args() + (L.dptr(agent._target_dev),)
                    else:
                        self._onecall_entry, tail = opt.onecall_tail()
                    self._onecall_args = (
                        L.dptr(pn.flat), L.dptr(tn.flat), L.dptr(r.old_iou), L.dptr(r.new_iou), L.dptr(r.ann), L.dptr(r.next_ann),
                        L.dptr(r.action), L.dptr(r.reward_step), L.dptr(r.reward_done), L.dptr(self.draw, torch.uint8), r.n, B, T,
                        float(np.float32(agent.GAMMA)), *agent._loss_args(), L.dptr(self.idx), L.dptr(self.state), L.dptr(self.new_state),
                        L.dptr(self.action), L.dptr(self.r_step), L.dptr(self.r_done), L.dptr(pn.flat_grad), L.dptr(self.loss), L.dptr(self.ws),
                        nbytes) + tail
                L.check(getattr(lib, self._onecall_entry)(*self._onecall_args, st), "dqn_step_drawn")
                continue
            if self.draw is not None:
                r.sample_drawn(B, self.draw, out=dict(idx=self.idx, state=self.state, new_state=self.new_state, action=self.action,
                                                      reward_step=self.r_step, reward_done=self.r_done))
            else:
                L.check(lib.ivosw_replay_gather(L.dptr(r.old_iou), L.dptr(r.new_iou), L.dptr(r.ann), L.dptr(r.next_ann),
                                                L.dptr(r.action), L.dptr(r.reward_step), L.dptr(r.reward_done), L.dptr(self.idx), B, T,
                                                L.dptr(self.state), L.dptr(self.new_state), L.dptr(self.action), L.dptr(self.r_step),
                                                L.dptr(self.r_done), st), "replay_gather")
            L.check(lib.ivosw_dqn_loss_grad_ex(L.dptr(pn.flat), L.dptr(tn.flat), L.dptr(self.state), L.dptr(self.new_state),
                                               L.dptr(self.action), L.dptr(self.r_step), L.dptr(self.r_done), B, T,
                                               float(np.float32(agent.GAMMA)), *agent._loss_args(), L.dptr(pn.flat_grad),
                                               L.dptr(self.loss), L.dptr(self.ws), nbytes, st), "dqn_loss_grad")
            if fused:
                opt.enqueue_dev_step()
            if self.tgt:
                agent.enqueue_target_update()

    def _hyper_now(self):
        """What the captured launches bake in: gamma and the loss option always (the loss); the optimizer's kind and values only when the
        update is part of the graph (fused) — the gradient-only graph of the data-parallel step leaves them to the eager update."""
        a = self.agent
        if not self.fused:
            return (float(a.GAMMA), a.loss_kind, float(a.huber_delta))
        per = self.replay.hyper() if self.per else ()
        return a.optimizer.hyper() + (float(a.optimizer.grad_scale), float(a.GAMMA), a.loss_kind, float(a.huber_delta)) + per + a.target_hyper()

    def launch(self):
        """Enqueue one step on the current stream; ``self.loss`` holds the device loss afterwards."""
        a = self.agent
        if self._keys != (a.policy_net.flat.data_ptr(), a.target_net.flat.data_ptr(), a.policy_net.flat_grad.data_ptr()):
            raise RuntimeError("the parameter arenas moved (.to() / re-pack) after capture: build a new CapturedDqnStep")
        if self._hyper != self._hyper_now():
            raise RuntimeError("a hyper-parameter (optimizer kind / lr / betas / eps / momentum / nesterov / weight_decay / clamp / grad_scale / "
                               "gamma / loss kind / huber_delta / lr schedule: lr_schedule, lr_pow, lr_total_steps / prioritized replay: "
                               "per_alpha, per_beta, per_beta_steps, per_eps / target rule: target_update, tau, target_period) changed after capture: the "
                               "graph replays the captured values - build a new CapturedDqnStep")
        if self.fused:
            a.optimizer.dev_state()              # resync if an eager step ran in between
        if self.tgt:
            a.target_dev_state()
        if self.graph is not None:
            self.graph.launch()
        else:
            self._enqueue()
        if self.fused:
            a.optimizer.note_dev_steps(self.steps)
        self.target_syncs = a.note_target_steps(self.steps) if self.tgt else 0      # hard syncs inside this launch (periodic)
        return self.loss


class GraphedDqnLoop:
    """The training loop of train_agent.py:177-182 / Agent.update_agent (models/agent.py:103-166) on captured graphs:
    every step = draw a minibatch, update the policy net, flip the reference's target-sync coin (``np.random.random() <
    update_rate``, one coin per step, in step order).  Steps are launched ``block`` at a time as ONE hipGraphLaunch whenever
    none of the block's coins fires (an 8.7 us bubble separates consecutive graph launches: per step it is 1/block of that);
    a block with a firing coin runs step by step with the sync where the reference has it.  Same coin stream, same minibatch
    stream (device counter), same arithmetic: results equal the step-by-step loop's bit for bit.
    Under agent.target_update = "soft" / "periodic" the rule is part of every captured step and no coin is drawn: EVERY full block is one
    graph launch, and ``syncs`` counts the hard syncs of the periodic rule (steps // period; 0 under soft)."""

    def __init__(self, agent, replay, B, draw_seed, block=8, draw_state=None):
        self.agent, self.block = agent, int(block)
        self.one = CapturedDqnStep(agent, replay, B, fused=True, draw_seed=draw_seed, draw_state=draw_state)
        self.many = CapturedDqnStep(agent, replay, B, fused=True, draw_state=self.one.draw, steps=self.block) if self.block > 1 else None
        self.launches = 0
        self.syncs = 0

    def run(self, n):
        """n training steps; returns the device loss tensor of the last one."""
        a = self.agent
        done, loss = 0, None
        while done < n:
            k = min(self.block, n - done)
            if self.one.tgt:                                       # the rule is inside the graphs: no host coin
                for st in ((self.many,) if k == self.block and self.many is not None else (self.one,) * k):
                    loss = st.launch()
                    self.launches += 1
                    self.syncs += st.target_syncs
                done += k
                continue
            coins = np.random.random(k) < a.update_rate            # the same draws, in the same order, as k scalar calls
            if k == self.block and self.many is not None and not coins.any():
                loss = self.many.launch()
                self.launches += 1
            else:
                for c in coins:
                    loss = self.one.launch()
                    self.launches += 1
                    if c:
                        a.sync_target()
                        self.syncs += 1
            done += k
        return loss


class LeanDqnLoop:
    """The same loop from PLAIN launches out of preallocated buffers (ivosw_dqn_step_drawn: encoder with the draw + gather, recurrence,
    decoder, head, BPTT, two tail launches, clamp + Adam with the slab reduction — eight launches per step, no graph; ten before round 4).  With the launch chain this short the host keeps ahead of the GPU (~190 us of GPU
    work per step) and the step loses the bubble that separates two graph launches; on a loaded host the captured loop is the
    safer choice (``AutoDqnLoop`` measures).  Same arithmetic, same coin and minibatch streams: bit-identical to the other loops."""

    def __init__(self, agent, replay, B, draw_seed, draw_state=None):
        self.agent, self.replay, self.B = agent, replay, B
        self.step = CapturedDqnStep(agent, replay, B, fused=True, draw_seed=draw_seed, draw_state=draw_state, capture=False)
        self.draw = self.step.draw
        self.syncs = 0

    def run(self, n):
        a, loss = self.agent, None
        for _ in range(n):
            loss = self.step.launch()               # ivosw_dqn_step_drawn: eight plain launches, the step counters on the device
            if self.step.tgt:                       # soft / periodic: the rule ran in the step's last launch
                self.syncs += self.step.target_syncs
            elif a.target_step():
                self.syncs += 1
        return loss


class AutoDqnLoop:
    """Runs the first steps once through each launch mode (captured blocks / plain launches), timed, and the rest through the
    faster one.  The probe steps are ordinary training steps and the modes are bit-identical, so the trajectory does not depend
    on the choice."""

    def __init__(self, agent, replay, B, draw_seed, block=8, probe=256):
        self.agent, self.probe = agent, int(probe)
        self.lean = LeanDqnLoop(agent, replay, B, draw_seed)
        self.graphed = GraphedDqnLoop(agent, replay, B, draw_seed, block=block, draw_state=self.lean.draw)
        self.choice, self.probe_us = None, {}

    def run(self, n):
        import time
        dev = torch.device(self.agent.device)
        loss = None
        if self.choice is None and n >= 2 * self.probe:
            for name, loop in (("graph", self.graphed), ("plain", self.lean), ("graph", self.graphed), ("plain", self.lean)):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                loss = loop.run(self.probe // 2)
                torch.cuda.synchronize(dev)
                self.probe_us[name] = min(self.probe_us.get(name, 1e30), (time.perf_counter() - t0) / (self.probe // 2) * 1e6)
            self.choice = min(self.probe_us, key=self.probe_us.get)
            n -= 2 * self.probe
        loop = self.lean if self.choice == "plain" else self.graphed
        if n > 0:
            loss = loop.run(n)
        return loss

    @property
    def syncs(self):
        return self.lean.syncs + self.graphed.syncs
