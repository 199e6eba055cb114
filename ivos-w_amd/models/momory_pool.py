"""Replay memory with the reference's class surface and CSV persistence format.

Mirrors /root/reference/models/momory_pool.py:8-162 (``Transition`` field order, ``ReplayMemory`` ring with
``position`` starting at -1, ``memory_pool.csv`` schema = index column + 12 columns, the per-sequence
``sample_th`` filter and the capacity shrink in ``load_from_csv``).  The module name keeps the reference's
spelling ("momory") so imports drop in.  ``DeviceReplay`` is the MI355X-side addition: the same rows as a
device-resident SoA that ``ivosw_replay_gather`` samples minibatches from.

Persistence.  The reference re-serialises the whole DataFrame through pandas on every push
(:126-153: O(N) per transition, ~100 MB of text at 50 k rows) and the dataset re-parses it every third sequence.
Here the CSV image is kept as pre-formatted text rows: ``push_to_csv`` formats ONE row, and the file is rewritten by a
single text join (no pandas) every ``csv_sync_every`` pushes (default 1 = the reference's behaviour: the file on disk is
byte-identical to the reference's after every push; at capacity every row's index label shifts, so the format itself
forbids a pure append).  Each sync also writes ``memory_pool.npz``, the same rows as a binary SoA that
``datasets.agent_dataset`` loads instead of re-parsing the text.
"""
import io
import os
import random
from collections import namedtuple

import numpy as np
import pandas as pd

Transition = namedtuple("Transition", ["state", "action", "next_state", "reward_step", "reward_done", "done",
                                       "state_iou", "next_state_iou", "annotated_frames", "next_annotated_frames"])

_CSV_COLUMNS = ("sequence", "scribble_iter", "n_interaction", "n_interaction_next", "action", "reward_step",
                "reward_done", "done", "state_iou", "next_state_iou", "annotated_frames", "next_annotated_frames")


def _mean_of_joined(strings):
    """'a/b/c' strings -> per-row mean (float64)."""
    return np.array([[float(tok) for tok in s.split("/")] for s in strings], dtype=np.float64).mean(axis=1)


class ReplayMemory:
    def __init__(self, capacity):
        self.capacity = capacity
        self.memory = []
        self.position = -1            # first push lands on slot 0
        self.basename_csv = "memory_pool.csv"
        self.COLUMNS = list(_CSV_COLUMNS)
        self._rows, self._label0, self._memory_pd = [], 0, None      # CSV image: text rows + first index label
        self._pending, self._needs_pandas, self._parsed = 0, False, {}
        self._col_kind = {}                        # pandas dtype of every numeric column of the image: int / float / object
        self.csv_sync_every = 1                    # 1 = rewrite memory_pool.csv on every push, like the reference
        self.seq_list = []

    def __len__(self):
        return len(self.memory)

    # ------------------------------------------------------------------ ring
    def push(self, *fields):
        if len(self.memory) < self.capacity:
            self.memory.append(None)
        self.position = (self.position + 1) % self.capacity
        self.memory[self.position] = Transition(*fields)

    def random_sample(self, batch_size):
        """Unused by the reference's training loop (minibatches come from the CSV), kept for the surface."""
        if batch_size > len(self.memory):
            return None
        picked = random.sample(self.memory, batch_size)
        return Transition(*zip(*picked))

    # ------------------------------------------------------------------ CSV
    def load_from_csv(self, path_to_random_memory_csv, report_save_dir=None, sample_th=0):
        frame = pd.read_csv(path_to_random_memory_csv, index_col=0)[:self.capacity]
        names = frame["sequence"].tolist()
        ordered_unique = list(dict.fromkeys(names))           # first-occurrence order
        if sample_th > 0:
            assert sample_th < 1
            self.seq_list = []
            for seq in ordered_unique:
                rows = frame[frame.sequence == seq]
                if len(rows) == 0:
                    continue
                lo = _mean_of_joined(rows.state_iou.values.tolist()).min()
                hi = _mean_of_joined(rows.next_state_iou.values.tolist()).max()
                if hi - lo > sample_th:
                    self.seq_list.append(seq)
            print(f"the number of available samples under threshold {sample_th}: {len(self.seq_list)}")
        else:
            self.seq_list.extend(ordered_unique)

        cols = {c: frame[c].tolist() for c in self.COLUMNS}
        kept = 0
        allowed = set(self.seq_list)
        for i in range(min(len(names), self.capacity)):
            if sample_th > 0:
                assert len(self.seq_list) > 0
                if names[i] not in allowed:
                    continue
            kept += 1
            where = dict(sequence=names[i], scribble_iter=cols["scribble_iter"][i])
            self.push(dict(where, n_interaction=cols["n_interaction"][i]), cols["action"][i],
                      dict(where, n_interaction=cols["n_interaction_next"][i]), cols["reward_step"][i],
                      cols["reward_done"][i], cols["done"][i], cols["state_iou"][i], cols["next_state_iou"][i],
                      cols["annotated_frames"][i], cols["next_annotated_frames"][i])
        self.capacity = kept           # the reference shrinks the ring to what it kept (:110)

        os.makedirs(report_save_dir, exist_ok=True)
        self.memory_pd = frame[:self.capacity]
        self.memory_pd.to_csv(os.path.join(report_save_dir, self.basename_csv))

    def _row_at(self, pos):
        t = self.memory[pos]
        return {"sequence": t.state["sequence"], "scribble_iter": t.state["scribble_iter"],
                "n_interaction": t.state["n_interaction"], "n_interaction_next": t.next_state["n_interaction"],
                "action": t.action, "reward_step": t.reward_step, "reward_done": t.reward_done, "done": t.done,
                "state_iou": t.state_iou, "next_state_iou": t.next_state_iou,
                "annotated_frames": t.annotated_frames, "next_annotated_frames": t.next_annotated_frames}

    # ---- CSV image as text rows -------------------------------------------------------------------------
    @staticmethod
    def _fmt(v):
        """One cell exactly as ``DataFrame.to_csv`` writes it (QUOTE_MINIMAL), or None if it would need quoting."""
        if isinstance(v, (bool, np.bool_)):
            return "True" if v else "False"
        if isinstance(v, (int, np.integer)):
            return str(int(v))
        if isinstance(v, (float, np.floating)):
            return "" if v != v else repr(float(v))
        t = str(v)
        return None if any(ch in t for ch in ',"\r\n') else t

    _NUMERIC = ("scribble_iter", "n_interaction", "n_interaction_next", "action", "reward_step", "reward_done")

    def _promote(self, col):
        """An int64 column that meets a typed float value becomes float64 for EVERY row, past and future: "0" is rewritten as "0.0"."""
        k = self.COLUMNS.index(col)
        out = []
        for r in self._rows:
            cells = r.split(",")
            c = cells[k]
            if c and "." not in c and "e" not in c and "n" not in c:       # an integer literal ('nan' / 'inf' stay)
                cells[k] = repr(float(int(c)))
            out.append(",".join(cells))
        self._rows = out
        self._parsed = {}

    def _format_row(self, row):
        """One CSV row as the reference's ``concat`` + ``to_csv`` (:139-152) would write it.  pandas types every numeric column
        of the pool: a one-row frame built from a python / numpy SCALAR is int64 or float64, one built from a 0-d ndarray
        (what ``agent_business`` passes for the rewards) is ``object``; concat gives int64 + float64 -> float64 (every row of
        the column is then written as a float, past rows included, and an int pushed later too), anything + object -> object
        (every cell keeps the text of its own type from then on)."""
        cells = []
        for c in self.COLUMNS:
            v = row[c]
            if c in self._NUMERIC and not isinstance(v, (bool, np.bool_)):
                if isinstance(v, np.ndarray) and v.ndim == 0:
                    kind, v = "object", v.item()
                elif isinstance(v, (float, np.floating)):
                    kind = "float"
                elif isinstance(v, (int, np.integer)):
                    kind = "int"
                else:
                    kind = "object"
                have = self._col_kind.get(c) if self._rows else None
                if have is None or have == kind:
                    now = kind
                elif "object" in (have, kind):
                    now = "object"
                else:
                    now = "float"                                  # int64 meets float64
                    if have == "int":
                        self._promote(c)
                    else:
                        v = float(v)
                if now == "float" and kind == "int":
                    v = float(v)
                self._col_kind[c] = now
            cells.append(self._fmt(v))
        return None if any(c is None for c in cells) else ",".join(cells)

    def _rows_from_frame(self, frame):
        """Text rows of a DataFrame exactly as pandas serialises them (labels stripped)."""
        lines = frame.to_csv().split("\n")[1:]
        return [ln.split(",", 1)[1] for ln in lines if ln]

    @property
    def memory_pd(self):
        """The reference's DataFrame image of the pool, materialised on demand from the text rows."""
        if self._memory_pd is None:
            text = "," + ",".join(self.COLUMNS) + "\n" + "".join(f"{self._label0 + i},{r}\n" for i, r in enumerate(self._rows))
            self._memory_pd = pd.read_csv(io.StringIO(text), index_col=0, float_precision="round_trip") if self._rows else pd.DataFrame(columns=self.COLUMNS)
        return self._memory_pd

    @memory_pd.setter
    def memory_pd(self, frame):
        self._memory_pd = frame
        self._rows = self._rows_from_frame(frame) if len(frame) else []
        self._label0 = int(frame.index.min()) if len(frame) else 0
        self._col_kind = {c: ("float" if str(frame[c].dtype).startswith("float") else "int" if str(frame[c].dtype).startswith("int") else "object")
                          for c in self._NUMERIC if c in frame.columns}

    def csv_text(self):
        return "," + ",".join(self.COLUMNS) + "\n" + "".join(f"{self._label0 + i},{r}\n" for i, r in enumerate(self._rows))

    def _write_csv(self, report_save_dir):
        os.makedirs(report_save_dir, exist_ok=True)
        path = os.path.join(report_save_dir, self.basename_csv)
        tmp = path + ".tmp"
        with open(tmp, "w") as f:
            f.write(self.csv_text())
        os.replace(tmp, path)                      # readers never see a half-written file
        self._pending = 0

    def sync_csv(self, report_save_dir, sidecar=True):
        """Write ``memory_pool.csv`` (byte-identical to the reference's file for the same push sequence) and, with
        ``sidecar``, the binary SoA image ``memory_pool.npz`` of the same rows (parsed rows are cached per text row)."""
        self._write_csv(report_save_dir)
        if not sidecar:
            return
        try:
            for r in self._rows:
                if r not in self._parsed:
                    self._parsed[r] = parse_text_rows([r])
            if len(self._parsed) > 2 * len(self._rows) + 64:
                live = set(self._rows)
                self._parsed = {k: v for k, v in self._parsed.items() if k in live}
            keys = ("action", "reward_step", "reward_done", "done", "old_state_iou", "new_state_iou", "annotated_frames",
                    "next_annotated_frames")
            soa = {k: np.concatenate([self._parsed[r][k] for r in self._rows]) for k in keys} if self._rows else parse_text_rows([])
            np.savez(os.path.join(report_save_dir, "memory_pool.npz"), nrows=np.int64(len(self._rows)),
                     sequence=np.array([r.split(",", 1)[0] for r in self._rows]), **soa)
        except Exception:                          # ragged / non-numeric rows: the CSV stays the source of truth
            pass

    def push_to_csv(self, report_save_dir):
        """Append the most recent transition to the CSV image, dropping the oldest row when over capacity
        (reference :126-153: concat with ignore_index, drop the smallest label, rewrite the file)."""
        line = self._format_row(self._row_at(self.position))
        if line is None or self._needs_pandas:
            # a cell needs CSV quoting: fall back to the reference's own pandas path for this pool
            self._needs_pandas = True
            row = pd.DataFrame(data={k: [v] for k, v in self._row_at(self.position).items()}, columns=self.COLUMNS)
            frame = pd.concat([self.memory_pd, row], ignore_index=True) if len(self.memory_pd) else row
            if len(frame) > self.capacity:
                frame = frame.drop(frame.index.min())
            self._memory_pd = frame
            os.makedirs(report_save_dir, exist_ok=True)
            frame.to_csv(os.path.join(report_save_dir, self.basename_csv))
            return
        self._rows.append(line)
        self._label0 = 0                           # concat(ignore_index=True) relabels from 0 ...
        if len(self._rows) > self.capacity:
            self._rows.pop(0)
            self._label0 = 1                       # ... and dropping label 0 leaves 1..capacity
        self._memory_pd = None
        self._pending += 1
        if self._pending >= self.csv_sync_every:
            # every push (the reference's cadence): text only; deferred cadence: also refresh the binary sidecar
            self.sync_csv(report_save_dir, sidecar=self.csv_sync_every > 1)


def parse_text_rows(rows):
    """Pre-formatted CSV rows (no label) -> the SoA dict of ``parse_rows`` without going through pandas."""
    cols = list(zip(*(r.split(",") for r in rows))) if rows else [[] for _ in _CSV_COLUMNS]
    by = dict(zip(_CSV_COLUMNS, cols))

    def mat(col):
        return np.array([[float(tok) for tok in s.split("/")] for s in by[col]], dtype=np.float64).reshape(len(rows), -1)
    return dict(action=np.array(by["action"], dtype=np.int64), reward_step=np.array(by["reward_step"], dtype=np.int64),
                reward_done=np.array(by["reward_done"], dtype=np.float64), done=np.array([d == "True" for d in by["done"]], dtype=bool),
                old_state_iou=mat("state_iou"), new_state_iou=mat("next_state_iou"),
                annotated_frames=mat("annotated_frames"), next_annotated_frames=mat("next_annotated_frames"))


def parse_rows(frame, T=None):
    """CSV frame -> SoA numpy dict (float64 [n,T] columns, int64/float64/bool scalars) — the arithmetic content
    of datasets/agent_dataset.py:71-115 without per-sample python objects."""
    def mat(col):
        return np.array([[float(tok) for tok in str(s).split("/")] for s in frame[col].tolist()], dtype=np.float64)
    out = dict(action=frame["action"].to_numpy(np.int64), reward_step=frame["reward_step"].to_numpy(np.int64),
               reward_done=frame["reward_done"].to_numpy(np.float64), done=frame["done"].to_numpy(bool),
               old_state_iou=mat("state_iou"), new_state_iou=mat("next_state_iou"),
               annotated_frames=mat("annotated_frames"), next_annotated_frames=mat("next_annotated_frames"))
    if T is not None:
        assert out["old_state_iou"].shape[1] == T
    return out


_M64 = (1 << 64) - 1


def draw_indices(seed, counter, B, n):
    """Host mirror of the device-side minibatch draw (``ivosw_replay_draw_gather``): the rows slot 0..B-1 of draw number
    ``counter`` read — a splitmix64 finaliser of (seed, counter, slot) scaled to [0, n) by the high half of a 64 x 64
    multiply.  Integer arithmetic only, so device, C host mirror (``ivosw_replay_draw_index``) and this agree bit for bit."""
    out = np.empty(B, dtype=np.int64)
    for b in range(B):
        z = (seed + 0x9E3779B97F4A7C15 * (counter + 1) + 0xD1B54A32D192ED03 * (b + 1)) & _M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        z ^= z >> 31
        out[b] = (z * n) >> 64
    return out


# ---------------------------------------------------------------------------------------------- prioritized replay (host side)
PER_N_MAX = 1 << 24               # rows of a prioritized replay (the device tree's limit)
PER_B_MAX = 1024                  # slots of one prioritized draw (one workgroup)


def per_params(alpha, beta0, beta_steps, eps):
    """(alpha, beta0, N_beta, eps), checked: alpha finite >= 0, beta0 in [0, 1], N_beta an int >= 0, eps finite > 0.  Anything else is a
    ValueError (named after the cfg.agent keys)."""
    num = lambda v: not isinstance(v, bool) and isinstance(v, (int, float, np.floating, np.integer))
    if not (num(alpha) and np.isfinite(alpha) and alpha >= 0):
        raise ValueError(f"agent.per_alpha must be a finite number >= 0, got {alpha!r}")
    if not (num(beta0) and 0 <= beta0 <= 1):
        raise ValueError(f"agent.per_beta must be a number in [0, 1], got {beta0!r}")
    if isinstance(beta_steps, bool) or not isinstance(beta_steps, (int, np.integer)) or not 0 <= beta_steps < 2 ** 31:
        raise ValueError(f"agent.per_beta_steps must be an int >= 0, got {beta_steps!r}")
    if not (num(eps) and np.isfinite(eps) and 0 < eps <= float(np.finfo(np.float32).max) and np.float32(eps) > 0):
        raise ValueError(f"agent.per_eps must be a finite number > 0, got {eps!r}")
    return float(alpha), float(beta0), int(beta_steps), float(eps)


def per_tree_leaves(n):
    """P: the next power of two >= max(n, 2); the tree of n rows is float32 [2P] (ivosw_per_tree_floats)."""
    P = 2
    while P < n:
        P <<= 1
    return P


def _draw_mix(seed, counter, b):
    z = (seed + 0x9E3779B97F4A7C15 * (counter + 1) + 0xD1B54A32D192ED03 * (b + 1)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def per_beta(beta0, beta_steps, counter):
    """beta of draw ``counter``: float32(beta0 + (1 - beta0) * (min(c, N) / N)), beta0 when N = 0 (the device's fp32 expression)."""
    f = np.float32
    if beta_steps == 0:
        return f(beta0)
    return f(f(beta0) + f(f(1) - f(beta0)) * f(f(min(int(counter), int(beta_steps))) / f(beta_steps)))


def per_draw_rows(tree, seed, counter, B, n):
    """Host mirror of the prioritized draw (``ivosw_per_draw_gather``) on a given tree (float32 [2P]): slot b of draw ``counter`` descends
    from the root with x = (total / B) * (b + u), u = float32(mix >> 40) * 2^-24, going left when x < the left child and right (x -= left)
    otherwise; the row is min(leaf - P, n - 1).  fp32 arithmetic throughout, as on the device."""
    f = np.float32
    tree = np.asarray(tree, dtype=np.float32)
    P = tree.shape[0] // 2
    step = f(tree[1] / f(B))
    out = np.empty(B, dtype=np.int64)
    for b in range(B):
        u = f(f(_draw_mix(seed & _M64, counter & 0xFFFFFFFF, b) >> 40) * f(2.0 ** -24))
        x = f(step * f(f(b) + u))
        node = 1
        while node < P:
            left = tree[2 * node]
            if x < left:
                node = 2 * node
            else:
                x = f(x - left)
                node = 2 * node + 1
        out[b] = min(node - P, n - 1)
    return out


def per_rebuild(tree):
    """Every internal node of a float32 tree [2P] recomputed from its leaves, float32(left + right) level by level (ivosw_per_build)."""
    t = np.array(tree, dtype=np.float32)
    lo = t.shape[0] // 4
    while lo >= 1:
        t[lo:2 * lo] = t[2 * lo:4 * lo:2] + t[2 * lo + 1:4 * lo:2]
        lo //= 2
    return t


def per_update_host(tree, max_priority, idx, td, alpha, eps, n):
    """Host mirror of ``ivosw_per_update`` -> (tree, max_priority): p_b = td_b + eps, the highest slot of a repeated row wins and sets
    its leaf to p_b ** alpha (float32), every ancestor of a touched leaf is recomputed from its children, and max_priority =
    max(max_priority, max_b p_b).  Rows outside [0, n) are skipped.  (numpy's float32 power stands in for the device's powf.)"""
    f = np.float32
    t = np.array(tree, dtype=np.float32)
    P = t.shape[0] // 2
    p = np.asarray(td, dtype=np.float32) + f(eps)
    last = {}
    for b, r in enumerate(np.asarray(idx, dtype=np.int64).tolist()):
        if 0 <= r < n:
            last[r] = b
    for r, b in last.items():
        t[P + r] = np.power(p[b], f(alpha), dtype=np.float32)
    nodes = {(P + r) >> 1 for r in last}
    while nodes:
        for i in nodes:
            t[i] = t[2 * i] + t[2 * i + 1]
        nodes = {i >> 1 for i in nodes if i > 1}
    return t, f(max(f(max_priority), p.max() if len(p) else f(max_priority)))


class DeviceReplay:
    """Device-resident SoA replay buffer; ``sample(idx)`` gathers a minibatch with ``ivosw_replay_gather``,
    ``sample_drawn`` draws the indices on the device as well (``ivosw_replay_draw_gather``)."""

    def __init__(self, soa, device):
        import torch
        from .. import _lib
        self._lib = _lib
        self.device = torch.device(device)
        f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(self.device).contiguous()
        self.old_iou, self.new_iou = f32(soa["old_state_iou"]), f32(soa["new_state_iou"])
        self.ann, self.next_ann = f32(soa["annotated_frames"]), f32(soa["next_annotated_frames"])
        self.action = torch.as_tensor(soa["action"], dtype=torch.int64).to(self.device)
        self.reward_step = f32(soa["reward_step"])
        self.reward_done = f32(soa["reward_done"])
        self.n, self.T = self.old_iou.shape

    def __len__(self):
        return self.n

    def sample(self, idx):
        """idx: int64 device tensor [B] -> dict of device tensors (state/new_state [B,T,2] fp32, ...)."""
        import torch
        L = self._lib
        B = idx.numel()
        state = torch.empty(B, self.T, 2, dtype=torch.float32, device=self.device)
        new_state = torch.empty_like(state)
        act = torch.empty(B, dtype=torch.int64, device=self.device)
        rs = torch.empty(B, dtype=torch.float32, device=self.device)
        rd = torch.empty_like(rs)
        L.check(L.lib().ivosw_replay_gather(
            L.dptr(self.old_iou), L.dptr(self.new_iou), L.dptr(self.ann), L.dptr(self.next_ann), L.dptr(self.action),
            L.dptr(self.reward_step), L.dptr(self.reward_done), L.dptr(idx, torch.int64), B, self.T,
            L.dptr(state), L.dptr(new_state), L.dptr(act), L.dptr(rs), L.dptr(rd), L.stream_ptr(self.device)),
            "replay_gather")
        return dict(state=state, new_state=new_state, action=act, reward_step=rs, reward_done=rd)

    def draw_state(self, seed, counter=0):
        """The 16-byte device state of the on-device draw: {uint64 seed, uint32 counter, uint32 owned by the library}."""
        import torch
        raw = np.zeros(2, dtype=np.uint64)
        raw[0] = np.uint64(seed & _M64)
        raw[1] = np.uint64(counter & 0xFFFFFFFF)
        assert self._lib.lib().ivosw_replay_draw_state_bytes() == raw.nbytes
        return torch.from_numpy(raw.view(np.uint8).copy()).to(self.device)

    def sample_drawn(self, B, draw_state, out=None):
        """Draw B rows on the device (advancing ``draw_state``'s counter) and gather them; ``out`` = preallocated dict with
        idx / state / new_state / action / reward_step / reward_done (what a captured graph records), else fresh tensors."""
        import torch
        L = self._lib
        if out is None:
            out = dict(idx=torch.empty(B, dtype=torch.int64, device=self.device),
                       state=torch.empty(B, self.T, 2, dtype=torch.float32, device=self.device),
                       new_state=torch.empty(B, self.T, 2, dtype=torch.float32, device=self.device),
                       action=torch.empty(B, dtype=torch.int64, device=self.device),
                       reward_step=torch.empty(B, dtype=torch.float32, device=self.device),
                       reward_done=torch.empty(B, dtype=torch.float32, device=self.device))
        L.check(L.lib().ivosw_replay_draw_gather(
            L.dptr(self.old_iou), L.dptr(self.new_iou), L.dptr(self.ann), L.dptr(self.next_ann), L.dptr(self.action),
            L.dptr(self.reward_step), L.dptr(self.reward_done), L.dptr(draw_state, torch.uint8), self.n, B, self.T,
            L.dptr(out["idx"], torch.int64), L.dptr(out["state"]), L.dptr(out["new_state"]), L.dptr(out["action"], torch.int64),
            L.dptr(out["reward_step"]), L.dptr(out["reward_done"]), L.stream_ptr(self.device)), "replay_draw_gather")
        return out


class PrioritizedReplay(DeviceReplay):
    """Prioritized experience replay (Schaul et al. 2016; cfg.agent.replay = "prioritized") over the same device SoA: a float32 sum tree
    [2P] whose leaf r is row r's priority ** alpha, and a 32-byte device state {uint64 seed, uint32 draw counter, float max_priority}.
    ``sample_prioritized`` draws a minibatch with P(row) = leaf / total (``ivosw_per_draw_gather``: stratified, on the device, the
    counter advances per call or graph replay) and returns the rows' importance-sampling weights; ``update_priorities`` sets the drawn
    rows' leaves from their TD errors (``ivosw_per_update``).  A fresh tree gives every row max_priority ** alpha (1 to begin with)."""

    def __init__(self, soa, device, alpha=0.6, beta0=0.4, beta_steps=0, eps=1e-6, seed=0, _carry=None):
        import torch
        super().__init__(soa, device)
        if not 1 <= self.n <= PER_N_MAX:
            raise ValueError(f"a prioritized replay holds 1 .. {PER_N_MAX} rows, got {self.n}")
        self.alpha, self.beta0, self.beta_steps, self.eps = per_params(alpha, beta0, beta_steps, eps)
        self.soa = soa
        lib = self._lib.lib()
        assert lib.ivosw_per_state_bytes() == 32
        self.P = per_tree_leaves(self.n)
        self.tree = torch.empty(int(lib.ivosw_per_tree_floats(self.n)), dtype=torch.float32, device=self.device)
        old, n_old = None, 0
        if _carry is not None:                    # rebuilt(): the draw state carries over, and the leaves when the rows are a prefix
            self.seed = _carry.seed
            self.state = _carry.state.clone()
            if _carry._is_prefix_of(soa):
                old, n_old = _carry.tree[_carry.P:_carry.P + _carry.n], _carry.n
        else:
            self.seed = int(seed) & _M64
            raw = np.zeros(4, dtype=np.uint64)
            raw[0] = np.uint64(self.seed)
            raw[2] = np.uint64(np.array([1.0], dtype=np.float32).view(np.uint32)[0])     # max_priority = 1.0 at byte 16
            self.state = torch.from_numpy(raw.view(np.uint8).copy()).to(self.device)
        L = self._lib
        L.check(lib.ivosw_per_build(L.dptr(self.tree), self.n, L.dptr(old) if old is not None else None, n_old, L.dptr(self.state),
                                    self._f32(self.alpha), L.stream_ptr(self.device)), "per_build")
        self.carried = n_old

    @staticmethod
    def _f32(v):
        return float(np.float32(v))

    def _is_prefix_of(self, soa):
        keys = ("old_state_iou", "new_state_iou", "annotated_frames", "next_annotated_frames", "action", "reward_step", "reward_done")
        for k in keys:
            a, b = np.asarray(self.soa[k]), np.asarray(soa[k])
            if b.shape[0] < a.shape[0] or a.shape[1:] != b.shape[1:] or a.dtype != b.dtype or not np.array_equal(a, b[:a.shape[0]]):
                return False
        return True

    def rebuilt(self, new_soa):
        """The replay over reloaded rows: the same options, seed, draw counter and max_priority; when the old rows are a prefix of the
        new ones (exact host comparison) their leaves are kept, otherwise every leaf starts again from max_priority ** alpha."""
        return PrioritizedReplay(new_soa, self.device, self.alpha, self.beta0, self.beta_steps, self.eps, _carry=self)

    def hyper(self):
        """What a captured step bakes in: (alpha, beta0, N_beta, eps) and the tree's address."""
        return (self.alpha, self.beta0, self.beta_steps, self.eps, self.tree.data_ptr(), self.state.data_ptr())

    def new_batch(self, B):
        """Preallocated outputs of ``sample_prioritized``: the minibatch dict plus idx, weights and td (filled by the weighted loss)."""
        import torch
        d = self.device
        return dict(idx=torch.empty(B, dtype=torch.int64, device=d), weights=torch.empty(B, dtype=torch.float32, device=d),
                    td=torch.zeros(B, dtype=torch.float32, device=d), state=torch.empty(B, self.T, 2, dtype=torch.float32, device=d),
                    new_state=torch.empty(B, self.T, 2, dtype=torch.float32, device=d), action=torch.empty(B, dtype=torch.int64, device=d),
                    reward_step=torch.empty(B, dtype=torch.float32, device=d), reward_done=torch.empty(B, dtype=torch.float32, device=d))

    def sample_prioritized(self, B, out=None):
        """Draw B rows by priority on the device (advancing the draw counter) and gather them; returns the minibatch dict with idx [B]
        int64, weights [B] fp32 (max 1) and a td [B] buffer; ``out`` = a dict from ``new_batch`` (what a captured graph records)."""
        import torch
        L = self._lib
        if not 1 <= B <= PER_B_MAX:
            raise ValueError(f"a prioritized draw takes 1 .. {PER_B_MAX} rows, got {B}")
        out = out if out is not None else self.new_batch(B)
        L.check(L.lib().ivosw_per_draw_gather(
            L.dptr(self.old_iou), L.dptr(self.new_iou), L.dptr(self.ann), L.dptr(self.next_ann), L.dptr(self.action),
            L.dptr(self.reward_step), L.dptr(self.reward_done), L.dptr(self.tree), L.dptr(self.state, torch.uint8), self.n, B, self.T,
            self._f32(self.beta0), self.beta_steps, L.dptr(out["idx"], torch.int64), L.dptr(out["weights"]), L.dptr(out["state"]),
            L.dptr(out["new_state"]), L.dptr(out["action"], torch.int64), L.dptr(out["reward_step"]), L.dptr(out["reward_done"]),
            L.stream_ptr(self.device)), "per_draw_gather")
        return out

    def update_priorities(self, idx, td):
        """Leaves of the rows ``idx`` [B] int64 <- (td + eps) ** alpha (the highest slot of a repeated row wins), ancestors rebuilt,
        max_priority raised; all on the device."""
        import torch
        L = self._lib
        L.check(L.lib().ivosw_per_update(L.dptr(self.tree), self.n, L.dptr(self.state, torch.uint8), L.dptr(idx, torch.int64), L.dptr(td),
                                         idx.numel(), self._f32(self.alpha), self._f32(self.eps), L.stream_ptr(self.device)), "per_update")

    # ---- host readers (synchronise) ----
    def tree_host(self):
        return self.tree.cpu().numpy()

    def leaves(self):
        return self.tree[self.P:self.P + self.n].cpu().numpy()

    def _state_host(self):
        return self.state.cpu().numpy()

    def counter(self):
        return int(self._state_host()[8:12].view(np.uint32)[0])

    def set_counter(self, c):
        import torch
        self.state[8:12].copy_(torch.from_numpy(np.array([c], dtype=np.uint32).view(np.uint8)))

    def max_priority(self):
        return float(self._state_host()[16:20].view(np.float32)[0])

    def beta_next(self):
        """beta of the next draw."""
        return float(per_beta(self.beta0, self.beta_steps, self.counter()))
