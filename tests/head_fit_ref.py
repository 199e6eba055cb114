"""ivosw_head_fit restated (include/ivosw.h, "THE STEP"): numpy in the dtype asked for - float32 follows the device's operation order and
rounding exactly, float64 is the yardstick - and the same loop written with real torch on the CPU (nn.Linear, the reference's per-sample
loss loop, backward, clamp_, optim.SGD), which measures what an fp32 implementation of the loop may lose against float64.

State of a fit: dict(w [2048], b, buf_w [2048], buf_b, grad_w [2048], grad_b, steps_taken), see ``fresh_state``."""
import numpy as np
import torch

C = 2048
_L = np.arange(64)


def fresh_state(w, b, dtype=np.float32):
    return dict(w=np.array(w, dtype=dtype).reshape(C).copy(), b=dtype(b), buf_w=np.zeros(C, dtype), buf_b=dtype(0), grad_w=np.zeros(C, dtype),
                grad_b=dtype(0), steps_taken=0)


def cast_state(st, dtype):
    return {k: (v if k == "steps_taken" else np.asarray(v, dtype=dtype).copy() if np.ndim(v) else dtype(v)) for k, v in st.items()}


def lr_table(lr0, gamma, num_epochs, steps_per_epoch):
    """lr0 * gamma**epoch in float64, rounded to fp32 once, repeated per step of the epoch: ExponentialLR stepped once per epoch."""
    per_epoch = np.array([float(lr0) * float(gamma) ** e for e in range(num_epochs)], dtype=np.float64).astype(np.float32)
    return np.repeat(per_epoch, steps_per_epoch)


def dots(X, w):
    """The row dots in the device's order: 64 lane partials over (j, q), then the xor butterfly.  X [B,2048], w [2048], one dtype."""
    prod = (X * w[None]).reshape(X.shape[0], 8, 64, 4)
    a = np.zeros((X.shape[0], 64), X.dtype)
    for j in range(8):
        for q in range(4):
            a = a + prod[:, j, :, q]
    for o in (32, 16, 8, 4, 2, 1):
        a = a + a[:, _L ^ o]
    return a[:, 0]


def run(feat, target, valid, order, lr, momentum, weight_decay, zero_grad, eval_only, state, dtype=np.float32, trace=None):
    """One fit: order [n_steps,B] row indices, lr [n_steps].  Returns (log [n_steps,3] in dtype, new state); ``state`` is not modified.
    Every input is cast to ``dtype`` first; every operation below is one rounded operation of that dtype.  ``trace``: a list that
    receives (step, channels clamped at +1, channels clamped at -1) of every step taken."""
    dt = np.dtype(dtype).type
    feat, target = np.asarray(feat, dtype=dt), np.asarray(target, dtype=dt)
    lr = np.asarray(lr, dtype=dt)
    mom, wd = dt(momentum), dt(weight_decay)
    st = cast_state(state, dt)
    w, b, buf_w, buf_b, G_w, G_b, taken = st["w"], st["b"], st["buf_w"], st["buf_b"], st["grad_w"], st["grad_b"], int(st["steps_taken"])
    order = np.asarray(order)
    log = np.zeros((order.shape[0], 3), dt)
    one, zero = dt(1), dt(0)
    for s, idx in enumerate(order):
        X = feat[idx]
        pred = dots(X, w) + b
        ok = np.asarray(valid)[idx] != 0
        c = int(ok.sum())
        if c == 0:
            continue
        e = pred - target[idx]
        S2, S1, Se, Sk = zero, zero, zero, np.zeros(C, dt)
        for n in range(len(idx)):
            if ok[n]:
                S2 = S2 + e[n] * e[n]
                S1 = S1 + np.abs(e[n])
                Se = Se + e[n]
                Sk = Sk + e[n] * X[n]
        cf = dt(c)
        log[s] = (S2 / cf, S1 / cf, cf)
        if eval_only:
            continue
        k = dt(2) / cf
        first = taken == 0

        def upd(S, p, buf, G):
            g = k * S
            G = (zero if zero_grad else G) + g
            if trace is not None and np.ndim(G):
                trace.append((s, int((G > one).sum()), int((G < -one).sum())))
            G = np.minimum(np.maximum(G, -one), one)
            d = G + wd * p
            buf = d if first else mom * buf + d
            return p - lr[s] * buf, buf, G
        w, buf_w, G_w = upd(Sk, w, buf_w, G_w)
        b, buf_b, G_b = upd(Se, b, buf_b, G_b)
        taken += 1
    return log, dict(w=w, b=dt(b), buf_w=buf_w, buf_b=dt(buf_b), grad_w=G_w, grad_b=dt(G_b), steps_taken=taken)


def torch_loop(feat, target, valid, order, lr, momentum, weight_decay, zero_grad, w0, b0, dtype=torch.float32, scheduler=None):
    """The reference's loop with real torch on the CPU from a fresh optimiser.  lr [n_steps] sets the rate of every step, unless
    ``scheduler`` = (lr0, gamma, steps_per_epoch): then torch's own ExponentialLR is stepped once per epoch.
    Returns (log [n_steps,3], w, b, grad_w, grad_b) as float64 numpy."""
    import torch.nn.functional as F
    lin = torch.nn.Linear(C, 1).to(dtype)
    with torch.no_grad():
        lin.weight.copy_(torch.as_tensor(np.asarray(w0, dtype=np.float64)).to(dtype).view(1, C))
        lin.bias.copy_(torch.as_tensor(np.asarray([b0], dtype=np.float64)).to(dtype))
    X, T = torch.as_tensor(np.asarray(feat)).to(dtype), torch.as_tensor(np.asarray(target)).to(dtype)
    lr0 = scheduler[0] if scheduler else float(lr[0])
    opt = torch.optim.SGD(lin.parameters(), lr=lr0, momentum=float(momentum), weight_decay=float(weight_decay))
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=scheduler[1]) if scheduler else None
    order = np.asarray(order)
    log = np.zeros((order.shape[0], 3))
    for s, idx in enumerate(order):
        if scheduler is None:
            for gr in opt.param_groups:
                gr["lr"] = float(lr[s])
        pred = lin(X[idx]).view(-1)
        loss, diff, counter = 0., 0., 0
        for n, i in enumerate(idx):
            if valid[i]:
                loss = loss + F.mse_loss(pred[n], T[i])
                diff = diff + (pred[n] - T[i]).abs().mean()
                counter += 1
        if counter:
            loss = loss / counter
            diff = diff / counter
            if zero_grad:
                opt.zero_grad()
            loss.backward()
            for p in lin.parameters():
                if p.grad is not None:
                    p.grad.data.clamp_(-1, 1)
            opt.step()
            log[s] = (loss.item(), diff.item(), counter)
        if sched is not None and (s + 1) % scheduler[2] == 0:
            sched.step()
    gw = lin.weight.grad.double().numpy().reshape(C).copy() if lin.weight.grad is not None else np.zeros(C)
    gb = float(lin.bias.grad.double()) if lin.bias.grad is not None else 0.0
    return log, lin.weight.detach().double().numpy().reshape(C).copy(), float(lin.bias.detach().double()), gw, gb


def within(got, want64, torch32, name=""):
    """The project's rule (the BPTT test): the device's error against float64 is at most 2 x the torch-fp32 loop's error against float64,
    or 1e-6 of the tensor's scale, whichever is larger.  Returns (error, bound) after asserting."""
    got, want64, torch32 = (np.asarray(v, dtype=np.float64) for v in (got, want64, torch32))
    err = float(np.abs(got - want64).max())
    bound = max(2.0 * float(np.abs(torch32 - want64).max()), 1e-6 * float(np.abs(want64).max()))
    print(f"{name}: device error {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (name, err, bound)
    return err, bound


def bank(M, seed, invalid=0.0, scale=1.0):
    """A synthetic non-negative feature bank (pooled ReLU outputs are >= 0), targets in [0, 1], validity flags."""
    rng = np.random.RandomState(seed)
    feat = (np.maximum(rng.standard_normal((M, C)), 0) * scale).astype(np.float32)
    target = rng.uniform(0, 1, M).astype(np.float32)
    valid = (rng.uniform(0, 1, M) >= invalid).astype(np.uint8)
    return feat, target, valid


def draw_order(M, B, n_epochs, seed):
    """The DataLoader's shuffle with drop_last: one permutation per epoch, cut into M // B batches of B."""
    rng = np.random.RandomState(seed)
    steps = M // B
    return np.concatenate([rng.permutation(M)[:steps * B].reshape(steps, B) for _ in range(n_epochs)]).astype(np.int32)


# ---------------------------------------------------------------------------------------------- shared fixtures
def clamp_case():
    """Gradients around the clamp on both sides: from w = 0, b = -0.25 the errors start near -0.75, features of scale 1.7 put |g| near 1,
    and a rate that overshoots turns the error's sign from step to step.  The bias starts away from zero on purpose: the rule's floor
    (1e-6 of the tensor's scale) exists to absorb rounding at the scale the numbers were computed at, and a scalar that ends as a
    cancellation residue far below its own history (b0 = 0 here ends near 2e-4 after visiting 1e-3) has a floor below one fp32 ulp of
    that history - no implementation that rounds every operation can be held to it.
    -> dict of run()'s arguments (momentum 0.9, weight decay, 2 epochs of 4 steps, B = 32)."""
    feat, target, valid = bank(128, 11, scale=1.7)
    order = draw_order(128, 32, 2, 5)
    return dict(feat=feat, target=target, valid=valid, order=order, lr=lr_table(6e-4, 0.5, 2, 4), momentum=0.9, weight_decay=5e-4,
                w0=np.zeros(C, np.float32), b0=-0.25)


def mixed_case():
    """Mixed validity, B = 17: about a third of the rows invalid; step 0 and step 3 hold invalid rows only (the reference's `continue`,
    once before any step was taken)."""
    feat, target, valid = bank(192, 12, invalid=0.35)
    order = draw_order(192, 17, 1, 6)[:6]
    bad = np.flatnonzero(valid == 0)
    order[0] = bad[:17]
    order[3] = bad[17:34]
    rng = np.random.RandomState(3)
    return dict(feat=feat, target=target, valid=valid, order=order, lr=lr_table(2e-4, 0.9, 2, 3), momentum=0.9, weight_decay=5e-4,
                w0=(rng.standard_normal(C) * 0.01).astype(np.float32), b0=0.1)
