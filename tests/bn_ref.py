"""Float64 references of the live-BatchNorm backbone (`--norm_layer_backbone batchnorm`), plain torch only on the CPU (nothing here
calls the HIP library): `F.batch_norm(training=True)` and torch.autograd.

`bn_act`       y = act(batch_norm(z) (+ residual)) over rows [M, C] with its statistics and torch's running-statistics update;
`bn_act_grads` gz, ggamma, gbeta, gres of it for a cotangent, by autograd;
`block_grads`  output, d/dx and every parameter gradient (convolution weights AND norm affines) of a chain of bottlenecks;
`body_taps` / `body_grads`  the five taps of the body in training mode (and the running statistics torch leaves behind) / every
               parameter gradient for one cotangent per tap."""
import torch
import torch.nn.functional as F

EPS, MOMENTUM = 1e-5, 0.1


def _d(t):
    return None if t is None else t.detach().double().cpu()


def bn_act(z, gamma, beta, run_mean=None, run_var=None, residual=None, relu=False, eps=EPS, momentum=MOMENTUM):
    """z [M, C] -> (y, mean, invstd, new run_mean, new run_var), float64; the running statistics are not modified in place."""
    z, gamma, beta, residual = _d(z), _d(gamma), _d(beta), _d(residual)
    rm = _d(run_mean).clone() if run_mean is not None else None
    rv = _d(run_var).clone() if run_var is not None else None
    if z.shape[0] > 1:
        y = F.batch_norm(z, rm, rv, gamma, beta, True, momentum, eps)
    else:       # torch refuses one value per channel; the definition: mean = z, biased variance 0, the running variance takes it as it is
        y = beta.expand_as(z).clone()
        if rm is not None:
            rm = (1 - momentum) * rm + momentum * z[0]
            rv = (1 - momentum) * rv
    mean = z.mean(0)
    invstd = 1.0 / torch.sqrt(z.var(0, unbiased=False) + eps) if z.shape[0] > 1 else torch.full_like(mean, 1.0 / eps ** 0.5)
    if residual is not None:
        y = y + residual
    return (F.relu(y) if relu else y), mean, invstd, rm, rv


def bn_act_grads(z, gamma, beta, cot, residual=None, relu=False, eps=EPS):
    """-> (gz, ggamma, gbeta, gres or None) of sum(y * cot), float64 autograd."""
    zd, gd, bd = (_d(t).requires_grad_(True) for t in (z, gamma, beta))
    rd = _d(residual).requires_grad_(True) if residual is not None else None
    y = F.batch_norm(zd, None, None, gd, bd, True, 0.0, eps)
    if rd is not None:
        y = y + rd
    if relu:
        y = F.relu(y)
    leaves = [zd, gd, bd] + ([rd] if rd is not None else [])
    g = torch.autograd.grad(y, leaves, _d(cot))
    return g[0], g[1], g[2], (g[3] if rd is not None else None)


# ------------------------------------------------------------------------------------------------ the body in training mode
def _leaves(sd, dtype=torch.float64):
    """leaves of `dtype` (float64: the reference; float32: what plain torch arithmetic itself reaches, the yardstick of the body tests):
    everything but the running statistics asks for a gradient."""
    out = {}
    for k, v in sd.items():
        stat = k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))
        out[k] = v.detach().cpu().clone() if k.endswith('num_batches_tracked') else v.detach().to(dtype).cpu().clone().requires_grad_(not stat)
    return out


def _bn(x, sd, p, stats=None):
    """NCHW train-mode BatchNorm; `stats` (dict): filled with torch's updated running statistics and the least batch variance."""
    rm, rv = sd[p + '.running_mean'].detach().clone(), sd[p + '.running_var'].detach().clone()
    y = F.batch_norm(x, rm, rv, sd[p + '.weight'], sd[p + '.bias'], True, MOMENTUM, EPS)
    if stats is not None:
        stats[p + '.running_mean'], stats[p + '.running_var'] = rm, rv
        stats['min_var'] = min(stats.get('min_var', float('inf')), float(x.detach().var((0, 2, 3), unbiased=False).min()))
    return y


def _relu(x, key, masks, record):
    """ReLU; `record` (dict): keeps its decisions (x > 0) under `key`, the name of the norm in front of it; `masks` (dict of NCHW bool
    tensors): the decisions are GIVEN -- y = x * mask -- so that the function differentiated is the one another evaluation (the kernels',
    float32 torch's) went through: where a value lies within rounding of zero, two precisions decide differently, and with a few dozen
    rows per channel one such disagreement moves a gradient by 1e-2 of its norm."""
    if record is not None:
        record[key] = x.detach() > 0
    return F.relu(x) if masks is None else x * masks[key].to(x.dtype)


def bottleneck(x, sd, p, stride, groups, dilation=1, stats=None, masks=None, record=None):
    """One bottleneck with live BatchNorm, NCHW float64; `p` = key prefix ('body.layer1.0')."""
    c = lambda name: sd[f'{p}.{name}.weight']
    o = _relu(_bn(F.conv2d(x, c('conv1')), sd, p + '.bn1', stats), p + '.bn1', masks, record)
    o = _relu(_bn(F.conv2d(o, c('conv2'), stride=stride, padding=dilation, dilation=dilation, groups=groups), sd, p + '.bn2', stats),
              p + '.bn2', masks, record)
    o = _bn(F.conv2d(o, c('conv3')), sd, p + '.bn3', stats)
    if f'{p}.downsample.0.weight' in sd:
        x = _bn(F.conv2d(x, c('downsample.0'), stride=stride), sd, p + '.downsample.1', stats)
    return _relu(o + x, p + '.bn3', masks, record)


def _taps(ld, img, layers, groups, dilation, stats, masks=None, record=None):
    x = F.conv2d(img.to(ld['init_conv.weight'].dtype), ld['init_conv.weight'], ld['init_conv.bias'])
    x = _relu(_bn(F.conv2d(x, ld['body.conv1.weight'], stride=2, padding=3), ld, 'body.bn1', stats), 'body.bn1', masks, record)
    taps = [x]
    x = F.max_pool2d(x, 3, 2, 1)
    for li, n in enumerate(layers, start=1):
        for bi in range(n):
            stride = 2 if (bi == 0 and li > 1 and not (dilation and li == 4)) else 1
            x = bottleneck(x, ld, f'body.layer{li}.{bi}', stride, groups, dilation=2 if (dilation and li == 4 and bi > 0) else 1,
                           stats=stats, masks=masks, record=record)
        taps.append(x)
    return taps


def block_grads(x, sd, blocks, groups, cotangent, dtype=torch.float64):
    """x [B,C,H,W] NCHW, blocks = [(key prefix, stride), ...] run one after the other, cotangent of the last output (NCHW)
    -> (output, d/dx, {key: gradient} of every convolution weight and norm affine), float64."""
    ld = _leaves(sd, dtype)
    xd = x.detach().to(dtype).cpu().requires_grad_(True)
    r = xd
    for p, s in blocks:
        r = bottleneck(r, ld, p, s, groups)
    keys = [k for k, v in ld.items() if v.requires_grad]
    grads = torch.autograd.grad(r, [xd] + [ld[k] for k in keys], cotangent.detach().to(dtype).cpu())
    return r.detach(), grads[0], dict(zip(keys, grads[1:]))


def body_taps(sd, img, layers, groups=1, dilation=False, dtype=torch.float64):
    """-> (five NCHW float64 taps of the training-mode forward, {key: running statistic after it, 'min_var': least batch variance})."""
    stats = {}
    with torch.no_grad():
        taps = _taps(_leaves(sd, dtype), img, layers, groups, dilation, stats)
    return taps, stats


def body_grads(sd, img, layers, cotangents, groups=1, dilation=False, dtype=torch.float64, masks=None, record=None):
    """sd: the `backbone.0.` part of a state_dict; loss = sum <tap_i, cotangent_i> -> (taps, {key: gradient}, stats), float64.
    `masks` / `record`: see `_relu`."""
    ld = _leaves(sd, dtype)
    stats = {}
    taps = _taps(ld, img, layers, groups, dilation, stats, masks, record)
    keys = [k for k, v in ld.items() if v.requires_grad]
    loss = sum((t * c.detach().to(dtype).cpu()).sum() for t, c in zip(taps, cotangents))
    grads = torch.autograd.grad(loss, [ld[k] for k in keys])
    return [t.detach() for t in taps], dict(zip(keys, grads)), stats
