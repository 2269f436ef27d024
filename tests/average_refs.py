"""numpy float32 definitions of csrc/average.hip — the bit-level definition of the kernels.  Every operation below is one correctly
rounded fp32 operation on np.float32 operands; nothing is fused."""
import numpy as np

F = np.float32


def ema_coef(decay, t):
    """c = max(1 - decay, 9 / (10 + t)), all in fp32; t = the step number after the tick (1 on the first step)."""
    return max(F(1.0) - F(decay), F(9.0) / (F(10.0) + F(t)))


def lerp(acc, x, c):
    """acc + c * (x - acc) as three separately rounded fp32 operations: subtract, multiply, add."""
    acc, x = np.asarray(acc, dtype=F), np.asarray(x, dtype=F)
    d = (x - acc).astype(F)
    s = (F(c) * d).astype(F)
    return (acc + s).astype(F)


def ema_run(masters_per_step, decay, start=None, t0=1):
    """The average after steps t0, t0 + 1, ...: it starts as ``start`` (default: the first snapshot — the optimiser copies the masters
    when the average is enabled, and steps only then) and folds in the masters as they are after each step."""
    ema = np.array(masters_per_step[0] if start is None else start, dtype=F, copy=True)
    for i, p in enumerate(masters_per_step):
        ema = lerp(ema, p, ema_coef(decay, t0 + i))
    return ema


def running_mean(xs, weights=None):
    """acc += (w_k / W_k) * (x_k - acc), W_k the running sum of the weights; the first input that carries weight initialises acc, an
    input of weight 0 is ignored (mtn_amd/average.py)."""
    weights = [1.0] * len(xs) if weights is None else list(weights)
    acc, w_sum = None, 0.0
    for x, w in zip(xs, weights):
        if w == 0:
            continue
        if acc is None:
            acc = np.array(x, dtype=F, copy=True)
        else:
            acc = lerp(acc, x, F(w / (w_sum + w)))
        w_sum += w
    return acc
