"""Float64 restatement of the EfficientNet-B0..B4 feature extractor (Tan & Le 2019; torchvision's module names), plain torch CPU ops only
(nothing here calls the HIP library or the product's backbone module): the stage table with its width / depth multipliers, one MBConv
block, the taps the detector reads, and the parameter count of the whole published network."""
import math

import torch
import torch.nn.functional as F

BASE = ((1, 3, 1, 32, 16, 1), (6, 3, 2, 16, 24, 2), (6, 5, 2, 24, 40, 2), (6, 3, 2, 40, 80, 3), (6, 5, 1, 80, 112, 3),
        (6, 5, 2, 112, 192, 4), (6, 3, 1, 192, 320, 1))            # (expand ratio, kernel, stride, in, out, repeats)
MULT = {'efficientnet_b0': (1.0, 1.0), 'efficientnet_b1': (1.0, 1.1), 'efficientnet_b2': (1.1, 1.2), 'efficientnet_b3': (1.2, 1.4),
        'efficientnet_b4': (1.4, 1.8)}
TAPS = (1, 2, 3, 5, 7)


def make_divisible(v, d=8):
    n = max(d, int(v + d / 2) // d * d)
    return n + d if n < 0.9 * v else n


def stages(name):
    w, dm = MULT[name]
    return [(t, k, s, make_divisible(i * w), make_divisible(o * w), int(math.ceil(n * dm))) for t, k, s, i, o, n in BASE]


def blocks(name):
    """[(stage index 1..7, block index, ratio, kernel, stride, in, out)] in order."""
    out = []
    for si, (t, k, s, i, o, n) in enumerate(stages(name), start=1):
        for bi in range(n):
            out.append((si, bi, t, k, s if bi == 0 else 1, i if bi == 0 else o, o))
    return out


def parameter_count(name, num_classes=1000):
    """Learnable parameters of the whole published network: stem, MBConv blocks, the 1x1 head convolution to 4 x the last width with its
    norm, and the classifier; two values per norm channel."""
    st = stages(name)
    n = 3 * st[0][3] * 9 + 2 * st[0][3]
    for _, _, t, k, _, cin, cout in blocks(name):
        cexp, csq = make_divisible(cin * t), max(1, cin // 4)
        if cexp != cin:
            n += cin * cexp + 2 * cexp
        n += cexp * k * k + 2 * cexp
        n += cexp * csq + csq + csq * cexp + cexp
        n += cexp * cout + 2 * cout
    last = st[-1][4]
    return n + last * 4 * last + 2 * 4 * last + 4 * last * num_classes + num_classes


def _bn(x, sd, p):
    s = sd[p + '.weight'].double() / torch.sqrt(sd[p + '.running_var'].double() + 1e-5)
    return x * s.view(1, -1, 1, 1) + (sd[p + '.bias'].double() - sd[p + '.running_mean'].double() * s).view(1, -1, 1, 1)


def silu(x):
    return x * torch.sigmoid(x)


def mbconv(x, sd, p, ratio, k, stride, cin, cout):
    """One block, NCHW float64; `p` = key prefix ('body.2.0')."""
    cexp = make_divisible(cin * ratio)
    o, i = x, 0
    if cexp != cin:
        o = silu(_bn(F.conv2d(o, sd[f'{p}.block.0.0.weight'].double()), sd, f'{p}.block.0.1'))
        i = 1
    o = silu(_bn(F.conv2d(o, sd[f'{p}.block.{i}.0.weight'].double(), stride=stride, padding=(k - 1) // 2, groups=cexp), sd, f'{p}.block.{i}.1'))
    se = f'{p}.block.{i + 1}'
    g = o.mean((2, 3), keepdim=True)
    g = silu(F.conv2d(g, sd[se + '.fc1.weight'].double(), sd[se + '.fc1.bias'].double()))
    g = torch.sigmoid(F.conv2d(g, sd[se + '.fc2.weight'].double(), sd[se + '.fc2.bias'].double()))
    o = _bn(F.conv2d(o * g, sd[f'{p}.block.{i + 2}.0.weight'].double()), sd, f'{p}.block.{i + 2}.1')
    return o + x if (stride == 1 and cin == cout) else o


def stem(sd, img):
    x = F.conv2d(img.double(), sd['init_conv.weight'].double(), sd['init_conv.bias'].double())
    return silu(_bn(F.conv2d(x, sd['body.0.0.weight'].double(), stride=2, padding=1), sd, 'body.0.1'))


def taps(sd, img, name):
    """sd: the `backbone.0.` part of a model state_dict; img [B,1,H,W] -> (stage-0 output, [five NCHW float64 taps])."""
    x0 = x = stem(sd, img)
    out = []
    for si, bi, t, k, s, cin, cout in blocks(name):
        x = mbconv(x, sd, f'body.{si}.{bi}', t, k, s, cin, cout)
        if si in TAPS and bi == stages(name)[si - 1][5] - 1:
            out.append(x)
    return x0, out
