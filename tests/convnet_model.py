"""A plain torch model of the conv-net executor's op list (prestage.Program): test infrastructure, not product code.

`interpret` runs a program on the CPU in float32 or float64 with ordinary torch ops, for any batch size: the reference
every executor test compares with.  `abs_conv` gives the magnitude term of the forward error bound of an f32 convolution.
"""
import torch
import torch.nn.functional as F

from dvd_amd import prestage

IN_EPS = 1e-5        # nn.InstanceNorm2d's default, what the executor uses


def add_conv(P, sd, a, cout, fill, ks=3, dil=1, relu=False, b=-1, stride=1):
    """Append a "plain" conv to program P and its tensors to the state dict sd: fill(name, shape) -> f32 tensor gives the
    weight [cout, cin, ks, ks] and the bias [cout].  Returns the destination slot."""
    name = f"c{len(P.convs)}"
    cin = P.ch[a] + (P.ch[b] if b >= 0 else 0)
    sd[name + ".weight"], sd[name + ".bias"] = fill(name + ".weight", (cout, cin, ks, ks)), fill(name + ".bias", (cout,))
    return P.conv(a, cout, ("plain", name + ".weight", name + ".bias"), ks, dil, 2 if relu else 0, b, stride)


def conv_params(program, weights, dtype=None):
    """{op index: (w [cout, cin, ks, ks], b [cout])} unpacked from a packed weight blob ([cout, kpad] tap-major, bias)."""
    out = {}
    convs = iter(program.convs)
    for i, o in enumerate(program.ops):
        if o["op"] != prestage.CONV:
            continue
        _, cin, cout, ks, kp = next(convs)
        off = o["w_off"]
        w = weights[off:off + cout * kp].reshape(cout, kp)[:, :ks * ks * cin].reshape(cout, ks, ks, cin).permute(0, 3, 1, 2)
        b = weights[off + cout * kp:off + cout * kp + cout]
        if dtype is not None:
            w, b = w.to(dtype), b.to(dtype)
        # fresh (aligned) storage, not views into the blob: torch's CPU kernels pick their vector path by alignment
        out[i] = (w.clone(memory_format=torch.contiguous_format), b.clone())
    return out


def _conv(o, inp, w, b):
    ks = w.shape[-1]
    return F.conv2d(inp, w, b, stride=2 if o.get("flag", 0) == 2 else 1, padding=o["dil"] * (ks // 2), dilation=o["dil"])


def instnorm(x, relu=False):
    """nn.InstanceNorm2d without affine: biased variance over h*w per image and channel, eps 1e-5."""
    y = F.instance_norm(x, eps=IN_EPS)
    return F.relu(y) if relu else y


def interpret(program, weights, x, dtype=torch.float32):
    """Run a prestage.Program on the CPU: x [N,C,H,W] -> {slot: tensor of `dtype`}."""
    params = conv_params(program, weights, dtype)
    slots = {0: x.to(dtype)}
    for i, o in enumerate(program.ops):
        a = slots[o["a"]]
        b = slots[o["b"]] if o.get("b", -1) >= 0 else None
        relu = o.get("act", 0) == 2
        if o["op"] == prestage.CONV:
            y = _conv(o, a if b is None else torch.cat((a, b), 1), *params[i])
            y = F.relu(y) if relu else y
        elif o["op"] == prestage.POOL:
            y = F.max_pool2d(a, 2, stride=2, ceil_mode=bool(o["flag"]))
        elif o["op"] == prestage.RESIZE:
            size = b.shape[2:] if b is not None else (o["h"], o["w"])
            y = F.interpolate(a, size=tuple(size), mode="bilinear", align_corners=bool(o["flag"]))
        elif o["op"] == prestage.ADD:
            y = F.relu(a + b) if relu else a + b
        elif o["op"] == prestage.SIGMOID:
            y = torch.sigmoid(a)
        elif o["op"] == prestage.INSTNORM:
            y = instnorm(a, relu)
        else:
            raise ValueError(f"op {i}: unknown kind {o['op']}")
        slots[o["dst"]] = y
    return slots


def abs_conv(program, weights, op, slots):
    """The convolution of op `op` applied to |x|, |w| and |b| in float64 (no activation): sum_k |x_k w_k| + |b| per output
    element, the magnitude in the forward error bound of a dot product.  `slots`: the float64 slots of `interpret`."""
    o = program.ops[op]
    w, b = conv_params(program, weights, torch.float64)[op]
    a = slots[o["a"]].double()
    inp = a if o.get("b", -1) < 0 else torch.cat((a, slots[o["b"]].double()), 1)
    return _conv(o, inp.abs(), w.abs(), b.abs())
