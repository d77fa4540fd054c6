"""Generates tests/golden/quant_w8.npz: the reference's own Quant_Conv2d, QuantBnConv2d and QuantDepthwiseNode at
weight_bit = 8 (pure PyTorch classes, CPU), imported the way make_golden.py imports them.  Arrays only.

  qconv_*   Quant_Conv2d(8, symmetric, per_channel): weights, bias, input, output
  qbn_*     QuantBnConv2d(8, symmetric, per_channel): conv weights, BN tensors, input, output
  head_*    QuantDepthwiseNode(8, 8, asymmetric activations, per_channel): the seven layers' tensors, two forwards
            (the "+=" initialisation and one EMA step of both QuantActs), outputs and tracked ranges

Usage:  python tests/golden/make_w8_golden.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import import_reference, t2n  # noqa: E402


def bn_of(c, g):
    b = nn.BatchNorm2d(c)
    b.weight.data = torch.rand(c, generator=g) + 0.5
    b.bias.data = torch.randn(c, generator=g) * 0.1
    b.running_mean = torch.randn(c, generator=g) * 0.1
    b.running_var = torch.rand(c, generator=g) + 0.5
    return b


def bn_arrays(prefix, bn, out):
    for k in ("weight", "bias", "running_mean", "running_var"):
        out["%s_%s" % (prefix, k)] = getattr(bn, k).detach().clone()


def main():
    _, ref_qm, _ = import_reference()
    g = torch.Generator().manual_seed(808)
    out = {}
    conv = nn.Conv2d(24, 4, 1, bias=True)
    conv.weight.data = torch.randn(4, 24, 1, 1, generator=g) * 0.3
    conv.bias.data = torch.randn(4, generator=g)
    qc = ref_qm.Quant_Conv2d(8, quant_mode="symmetric", per_channel=True)
    qc.set_param(conv)
    x = torch.randn(1, 24, 3, 3, generator=g)
    out.update(qconv_w=conv.weight.data, qconv_b=conv.bias.data, qconv_x=x, qconv_y=qc(x))

    conv2 = nn.Conv2d(40, 3, 1, bias=False)
    conv2.weight.data = torch.randn(3, 40, 1, 1, generator=g) * 0.1
    bn = bn_of(3, g)
    qb = ref_qm.QuantBnConv2d(8, quant_mode="symmetric", per_channel=True)
    qb.set_param(conv2, bn)
    x2 = torch.randn(1, 40, 2, 2, generator=g)
    out.update(qbn_w=conv2.weight.data, qbn_x=x2, qbn_y=qb(x2))
    bn_arrays("qbn_bn", bn, out)

    C, ncls = 8, 2
    seq = nn.Sequential(nn.Conv2d(C, C, 1, bias=False), bn_of(C, g), nn.ReLU(inplace=True),
                        nn.Conv2d(C, C, 3, 1, 1, groups=C, bias=False), bn_of(C, g), nn.ReLU(inplace=True),
                        nn.Conv2d(C, ncls, 1, bias=True)).eval()
    seq[0].weight.data = torch.randn(C, C, 1, 1, generator=g) * (1.5 / C) ** 0.5
    seq[3].weight.data = torch.randn(C, 1, 3, 3, generator=g) / 3
    seq[6].weight.data = torch.randn(ncls, C, 1, 1, generator=g) * (1.0 / C) ** 0.5
    seq[6].bias.data = torch.randn(ncls, generator=g) * 0.1
    out.update(head_w1=seq[0].weight.data.clone(), head_w2=seq[3].weight.data.clone(),
               head_w3=seq[6].weight.data.clone(), head_b3=seq[6].bias.data.clone())
    bn_arrays("head_bn1", seq[1], out)
    bn_arrays("head_bn2", seq[4], out)
    node = ref_qm.QuantDepthwiseNode(8, 8, act_percentile=False, wt_quant_mode="symmetric", act_quant_mode="asymmetric",
                                     per_channel=True, weight_percentile=False)
    node.set_param(seq)
    node.eval()
    for it in range(2):
        xh = torch.randn(1, C, 4, 4, generator=g).abs() * (1.0 + 0.5 * it)
        with torch.no_grad():
            yh = node(xh)
        out["head_x%d" % it] = xh
        out["head_y%d" % it] = yh
        for name, act in (("a1", node.quant_act1[1]), ("a3", node.quant_act3[1])):
            out["head_%s_min%d" % (name, it)] = act.x_min.clone()
            out["head_%s_max%d" % (name, it)] = act.x_max.clone()
    np.savez_compressed(os.path.join(HERE, "quant_w8.npz"), **t2n(out))
    print("wrote quant_w8.npz (%d arrays)" % len(out))


if __name__ == "__main__":
    main()
