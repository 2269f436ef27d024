#!/usr/bin/env python
"""Checkpoint averaging: the weighted mean of several checkpoints in weight space, as one checkpoint that decodes at one model's cost.

    python average.py --inputs exp/mtn_11 exp/mtn_12 exp/mtn_13 --output exp/mtn_avg [--weights 1 1 2]

Prefixes are given as for generate.py's --model (<prefix>.pth.tar = a state_dict in the reference's key schema).  The checkpoints are
loaded one at a time; every floating-point entry lives in ONE flat fp32 accumulator on the device (each entry at a multiple of 4
elements) and checkpoint k is folded in by one launch of mtn_lerp_f32 (csrc/average.hip):

    acc += (w_k / W_k) * (x_k - acc),    W_k = w_1 + ... + w_k

— the running weighted mean, three separately rounded fp32 operations per element (tests/average_refs.py running_mean is its numpy
definition).  The first checkpoint that carries weight initialises the accumulator; a checkpoint of weight 0 is checked and otherwise
ignored.  Integer and boolean entries must be equal in every input and are copied.
"""
import argparse
import math

import numpy as np
import torch

from . import lib as L


def weights_error(weights, n_inputs):
    """What is wrong with the weights, as one line (None: nothing)."""
    if len(weights) != n_inputs:
        return "--weights takes one weight per --inputs entry (%d given for %d)" % (len(weights), n_inputs)
    for i, w in enumerate(weights):
        if not math.isfinite(w):
            return "weight %d is not finite (%r)" % (i, w)
        if w < 0:
            return "weight %d is negative (%r)" % (i, w)
    if not any(w > 0 for w in weights):
        return "the weights are all zero"
    return None


def parse(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--inputs", nargs="+", required=True, metavar="PREFIX", help="checkpoint prefixes (<prefix>.pth.tar), as generate.py's --model")
    p.add_argument("--output", required=True, metavar="PREFIX", help="the mean is written to <prefix>.pth.tar")
    p.add_argument("--weights", nargs="+", type=float, default=None, help="one weight >= 0 per input, not all 0 (default: uniform)")
    p.add_argument("--gpu", "-g", default=0, type=int)
    args = p.parse_args(argv)
    if args.weights is None:
        args.weights = [1.0] * len(args.inputs)
    err = weights_error(args.weights, len(args.inputs))
    if err:
        p.error(err)
    return args


def _layout(sd):
    """[(key, offset, numel)] of the floating-point entries in the flat buffer (every entry starts at a multiple of 4 elements), total"""
    lay, total = [], 0
    for k, v in sd.items():
        if v.is_floating_point():
            lay.append((k, total, v.numel()))
            total += (v.numel() + 3) // 4 * 4
    return lay, total


def _check_against(first, sd, name_first, name):
    """SystemExit naming the first key that ``sd`` lacks, that only ``sd`` has, or whose shape or dtype differs from ``first``'s."""
    for k, v in first.items():
        if k not in sd:
            raise SystemExit("average: key %r of %s is missing from %s" % (k, name_first, name))
        u = sd[k]
        if tuple(u.shape) != tuple(v.shape):
            raise SystemExit("average: key %r has shape %s in %s and %s in %s" % (k, tuple(u.shape), name, tuple(v.shape), name_first))
        if u.dtype != v.dtype:
            raise SystemExit("average: key %r has dtype %s in %s and %s in %s" % (k, u.dtype, name, v.dtype, name_first))
        if not v.is_floating_point() and not torch.equal(u, v):
            raise SystemExit("average: the %s entry %r differs between %s and %s: only floating-point entries are averaged" % (v.dtype, k, name_first, name))
    for k in sd:
        if k not in first:
            raise SystemExit("average: key %r of %s is missing from %s" % (k, name, name_first))


def _flat(sd, lay, total):
    x = torch.zeros(total, dtype=torch.float32)
    for k, o, n in lay:
        x[o:o + n].copy_(sd[k].reshape(-1))
    return x


def average_state_dicts(load, names, weights, device):
    """The weighted mean of the state dicts ``load(name)`` returns, for name in ``names``: one is held at a time.  Returns a state dict of
    CPU tensors with the first input's keys, shapes and dtypes."""
    err = weights_error(weights, len(names))
    if err:
        raise SystemExit("average: " + err)
    first = load(names[0])
    lay, total = _layout(first)
    acc = x = None
    w_sum = 0.0
    for i, (name, w) in enumerate(zip(names, weights)):
        sd = first if i == 0 else load(name)
        if i > 0:
            _check_against(first, sd, names[0], name)
        if w == 0 or total == 0:
            continue
        if acc is None:                    # the first checkpoint that carries weight is the mean so far
            acc = _flat(sd, lay, total).to(device)
            x = torch.empty_like(acc)
        else:
            x.copy_(_flat(sd, lay, total))
            L.check(L.load().mtn_lerp_f32(total, acc.data_ptr(), x.data_ptr(), float(np.float32(w / (w_sum + w))), L.stream_ptr()))
        w_sum += w
    out = {}
    mean = acc.cpu() if acc is not None else None
    offs = {k: (o, n) for k, o, n in lay}
    for k, v in first.items():
        if k in offs:
            o, n = offs[k]
            out[k] = mean[o:o + n].view(v.shape).to(v.dtype).clone()
        else:
            out[k] = v.clone()
    return out


def main(argv=None):
    args = parse(argv)
    from .generate import load_state_dict
    if not torch.cuda.is_available():
        raise SystemExit("average: no GPU (the accumulation runs on the device; there is no CPU path)")
    dev = torch.device("cuda", args.gpu)
    torch.cuda.set_device(dev)
    out = average_state_dicts(lambda prefix: load_state_dict(prefix + ".pth.tar"), list(args.inputs), list(args.weights), dev)
    torch.save(out, args.output + ".pth.tar")
    print("average: %d checkpoint(s), weights %s -> %s.pth.tar (%d entries)" % (len(args.inputs), args.weights, args.output, len(out)))


if __name__ == "__main__":
    main()
