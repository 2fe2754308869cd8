"""Weight-layout preparation for the HIP kernels.

Checkpoints keep the reference layout (conv weight [Cout, Cin, kh, kw]); the implicit-GEMM kernel
wants KRSC rows [Cout, kh*kw*Cin] (k contiguous, padded to a multiple of 32 floats when Cin is not).
Prepared copies are cached per parameter and invalidated by torch's version counter.
"""
import weakref

import torch
import torch.nn.functional as F

_cache = {}         # (id(tensor), tag) -> (weakref to the tensor, version tuple, prepared value)
_epoch = 0          # bumped whenever a kernel rewrote parameters / buffers through raw pointers


def bump():
    """Invalidate every prepared copy: the fused optimiser and the train-mode BatchNorm kernels update tensors in
    place through raw pointers, which torch's version counters cannot see."""
    global _epoch
    _epoch += 1


_DEBUG = __import__('os').environ.get('NBM_PREP_DEBUG') == '1'


def _evict(obj_id):
    for k in [k for k in _cache if k[0] == obj_id]:
        hit = _cache.pop(k, None)
        if _DEBUG and hit is not None:
            v = hit[2]
            ts = [t for t in (v if isinstance(v, (tuple, list)) else [v]) if torch.is_tensor(t)]
            print(f'_prep: evicted {k[1]} (key tensor died), values at {[hex(t.data_ptr()) for t in ts]}', flush=True)


def _cached(key_t, tag, fn, extra=(), epoch=True):
    """Prepared copy of `key_t`.  An entry belongs to ONE tensor object: it keeps a weak reference to it and is only
    valid while that referent is alive and is `key_t` itself -- CPython reuses ids and the caching allocator reuses
    device addresses, so (id, data_ptr, version) alone can match a different model's parameter after the first model was
    freed.  Entries are dropped when their tensor dies (the prepared copies would otherwise leak on the device)."""
    key = (id(key_t), tag)
    # `epoch=False`: the inputs are buffers that no kernel ever writes through a raw pointer (FrozenBatchNorm): torch's own version
    # counters see every change they can undergo (load_state_dict, .to()), so the entry outlives the optimiser steps
    ver = (key_t.data_ptr(), key_t._version, key_t.device, _epoch if epoch else -1) + tuple(extra)
    hit = _cache.get(key)
    if hit is not None and hit[0]() is key_t and hit[1] == ver:
        return hit[2]
    with torch.no_grad():
        val = fn()
    if _DEBUG:
        cap = torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()
        print(f'_prep: made {tag} for a {tuple(key_t.shape)} key (replaces an entry: {hit is not None}; during a capture: {cap})', flush=True)
    obj_id = id(key_t)
    _cache[key] = (weakref.ref(key_t, lambda _r, obj_id=obj_id: _evict(obj_id)), ver, val)
    return val


def krsc(weight):
    """[Cout, Cin, kh, kw] -> contiguous [Cout, K'] with K' = kh*kw*Cin rounded up to 32 when Cin % 32 != 0."""
    def make():
        co, ci, kh, kw = weight.shape
        w = weight.detach().permute(0, 2, 3, 1).reshape(co, kh * kw * ci)
        if ci % 32:
            w = F.pad(w, (0, (-w.shape[1]) % 32))
        return w.contiguous()
    return _cached(weight, 'krsc', make)


def _gconv_fragments(weight, groups):
    C, Cg, kh, kw = weight.shape
    if (kh, kw) != (3, 3) or C != groups * Cg or 16 % min(Cg, 16) or Cg % 16 not in (0, Cg) or C % 16:
        raise ValueError(f'gconv: no fragment layout for a {tuple(weight.shape)} weight in {groups} groups')
    w = weight.reshape(C, Cg, 9)
    CI = max(Cg, 16)
    if Cg < 16:
        # row n of the 16-channel slab that holds its group: columns ci with ci // Cg == (n % 16) // Cg carry W[n][ci % Cg]
        same = (torch.arange(16, device=w.device)[None, :] // Cg) == ((torch.arange(C, device=w.device) % 16) // Cg)[:, None]
        w = w.repeat(1, 16 // Cg, 1) * same[:, :, None].to(w.dtype)
    # [C, CI, 9] -> (t, n % 16, j, q, e, tap) -> (t, tap, j, q, n % 16, e)
    return w.reshape(C // 16, 16, CI // 16, 4, 4, 9).permute(0, 5, 2, 3, 1, 4).reshape(C // 16, 9, CI // 16, 64, 4).contiguous()


def gconv(weight, groups):
    """Grouped 3x3 weights [C, Cg, 3, 3] (checkpoint layout, C = groups * Cg) -> the fragment order of `nbm_gconv3x3`
    (include/nbm_hip.h): [C / 16][9][CI / 16][64][4] with CI = max(Cg, 16), element (t, 3 r + s, j, lane, e) = W[n][ci - g(n) Cg][r][s]
    for n = 16 t + (lane & 15) and the input channel ci = (16 t // CI) CI + 16 j + 4 (lane >> 4) + e when ci lies in n's group g(n),
    else 0 -- groups narrower than 16 channels share a 16 x 16 fragment as a block diagonal."""
    return _cached(weight, ('gconv', int(groups)), lambda: _gconv_fragments(weight.detach(), groups))


def dw_taps(weight):
    """Depthwise weights [C, 1, k, k] (checkpoint layout) -> tap-major [k * k, C] for `nbm_dwconv_bn_act` (16-byte loads along C)."""
    return _cached(weight, 'dwtaps', lambda: weight.detach().reshape(weight.shape[0], -1).t().contiguous())


def gconv_dgrad(weight, groups, scale=None):
    """The weights of the DATA-GRADIENT convolution of a grouped 3x3 layer (`nbm_gconv3x3_dgrad`), in the fragment order of `gconv`:
    transposed inside each group, rotated by 180 degrees, and with the FrozenBN `scale` [C] that multiplies the incoming gradient per
    output channel folded in (the pattern of `wino23(transposed=True, scale=)`):
        W'[g Cg + c][n][r][s] = scale[g Cg + n] * W[g Cg + n][c][2 - r][2 - s]."""
    def make():
        C, Cg, kh, kw = weight.shape
        if (kh, kw) != (3, 3) or C != groups * Cg:
            raise ValueError(f'gconv_dgrad: no fragment layout for a {tuple(weight.shape)} weight in {groups} groups')
        w = weight.detach().reshape(groups, Cg, Cg, 3, 3)
        if scale is not None:
            w = w * scale.detach().reshape(groups, Cg, 1, 1, 1)
        return _gconv_fragments(w.transpose(1, 2).flip(3, 4).reshape(C, Cg, 3, 3), groups)
    # the scale's identity belongs to the entry's VERSION, not to its key (see wino23)
    extra = () if scale is None else (scale.data_ptr(), scale._version)
    return _cached(weight, ('gconv_dgrad', int(groups), scale is not None), make, extra=extra)


def wino23(weight, transposed=False, m=2, scale=None):
    """Winograd F(m x m, 3x3) weights U[(m+2)^2][N][C] = (G g G^T)[i][j] of a [Cout, Cin, 3, 3] convolution (`nbm_wino_weight`:
    float64 arithmetic on the device, rounded once).  `transposed`: the weights of the DATA-GRADIENT convolution (kernel
    rotated by 180 degrees, channel roles swapped): U[..][Cin][Cout]; `scale` [Cout] (transposed only): the FrozenBN scale
    that multiplies the incoming gradient per output channel, folded into the weights."""
    from .. import ops

    def make():
        return ops.wino_weight(weight.detach().contiguous(), transposed, m, None if scale is None else scale.detach().contiguous())
    # ONE entry per (weight, m, transposed, scaled?): the scale's identity is part of the entry's VERSION, not of its key -- the
    # FrozenBN affine is a fresh tensor every forward pass, so a key holding its data_ptr added a 36-plane copy per layer and step
    # that nothing evicted (60-130 MB per training step: scripts/soak.py)
    extra = () if scale is None else (scale.data_ptr(), scale._version)
    return _cached(weight, ('wino', m, transposed, scale is not None), make, extra=extra)


def wino23_weight_grad(dU, m=2, row_scale=None):
    """dU [(m+2)^2, N, C] (gradient wrt the transformed weights) -> dW [N, C, 3, 3] = row_scale[n] G^T dU G."""
    from .. import ops
    return ops.wino_weight_grad(dU, m, row_scale)


def cell_weight(weight, forward=False):
    """Kernel side of the cell transforms (csrc/cellwino.hip, `nbm_cell_weight`): [Cout, Cin, 3, 3] -> U [25][Cin][Cout] =
    (E w E^T)[a][b] -- the B operand of the 25 data-gradient GEMMs M_xi = Vg_xi U_xi^T; `forward`: [25][Cout][Cin], the B operand of
    the forward GEMMs M_xi = Vx_xi U_xi^T.  float64 on the device, rounded once; cached per weight version."""
    from .. import ops
    return _cached(weight, ('cell', forward), lambda: ops.cell_weight(weight.detach().contiguous(), forward=forward))


def cell_weight_folded(w_out, wk_lat, alpha, transposed=False):
    """B operand of the cell-domain plane GEMMs of a demand-driven 3x3 convolution whose lateral was deferred
    (ondemand.conv1x1_lazy(defer=True)): [25][N][C + Cin] = [ U | alpha * U W_lat ] with U = E w_out E^T ([25][N][C]) and
    W_lat = wk_lat the lateral's KRSC weights [C][Cin] -- the merged map x = alpha * W_lat t + b + up(x1) never exists
    on the pattern patches: its transform is [transform(up(x1) + b) | transform(t)].  `transposed`: the same values as
    [25][C + Cin][N], the B operand of the data-gradient GEMMs (rows C.. give d/dt in the transform domain).  Both layouts come out
    of one pair of launches (`nbm_cell_weight` + `nbm_cell_weight_fold`) and share the cache entry."""
    from .. import ops
    pair = _cached(w_out, ('cellfold', float(alpha)),
                   lambda: ops.cell_weight(w_out.detach().contiguous(), lateral=wk_lat.detach(), alpha=alpha, both=True),
                   extra=(wk_lat.data_ptr(), wk_lat._version, tuple(wk_lat.shape)))
    return pair[1] if transposed else pair[0]


def cell_weight_grad(dU):
    """dU [25][N][C] (gradient wrt the transformed kernel) -> dW [N, C, 3, 3] = E^T dU E (`nbm_cell_weight_grad`)."""
    from .. import ops
    return ops.cell_weight_grad(dU)


def stem_fold(w1, w_init, b_init):
    """Operands of `nbm_stem7x7`: init_conv (1 -> 3 channels, weight a_c, bias b_c) folded into conv1 [64,3,7,7], in float64:
    weff [56,64] (k = 8 r + s, the s = 7 column zero) = sum_c W1 a_c; wb [64,49] = sum_c W1 b_c; wb_full [64] = wb.sum(1)."""
    def make():
        w = w1.detach().double()
        a, b = w_init.detach().double().view(3), b_init.detach().double().view(3)
        we = (w * a.view(1, 3, 1, 1)).sum(1)                       # [64,7,7]
        wb = (w * b.view(1, 3, 1, 1)).sum(1)
        weff = torch.zeros((7, 8, 64), dtype=torch.float64, device=w.device)
        weff[:, :7] = we.permute(1, 2, 0)
        return (weff.view(56, 64).float().contiguous(), wb.reshape(64, 49).float().contiguous(), wb.sum((1, 2)).float().contiguous())
    return _cached(w1, 'stem', make, extra=(w_init.data_ptr(), w_init._version, b_init.data_ptr(), b_init._version))


def bn_affine(weight, bias, mean, var, eps, conv_bias=None, frozen=False):
    """Fold (conv bias +) BatchNorm running statistics into per-channel (scale, shift):
    y = (z + conv_bias - mean) * weight / sqrt(var + eps) + bias  =  z * scale + shift."""
    def make():
        scale = weight.detach() * (var + eps).rsqrt()
        shift = bias.detach() - mean * scale
        if conv_bias is not None:
            shift = shift + conv_bias.detach() * scale
        return scale.contiguous(), shift.contiguous()
    # any of the five tensors changing must invalidate: their versions are part of the entry's version (`extra`), NOT of its key -- a
    # key that changes with every update would leave one stale entry per update behind
    extra = (weight._version, bias._version, mean._version, var._version, None if conv_bias is None else conv_bias._version,
             mean.data_ptr(), var.data_ptr(), bias.data_ptr())
    # `frozen` (backbone.FrozenBatchNorm2d): the 53 affines of the ResNet body used to be recomputed after EVERY optimiser step (five
    # pointwise launches each: 265 of the ~650 small torch launches of a training step, scripts/small_launches.py) because the step
    # invalidates every prepared copy; their four tensors are buffers nothing writes behind torch's back
    return _cached(weight, ('bn', conv_bias is not None), make, extra=extra, epoch=not frozen)


def _rpn_composite64(out_w, out_b, dw_w, dw_b, pt_w, rmask, smask, lat_wk, alpha):
    """float64: (W_eff [N][5][5][K], const [N]) of `rpn_composite` for one class of cells."""
    n1, c = out_w.shape[0], out_w.shape[1]
    m_ = dw_w.shape[0]
    mult = m_ // n1
    wo = out_w.detach().double().repeat_interleave(mult, 0)              # [M, C, 3, 3]: depthwise channel m reads out_conv channel m // mult
    wd = dw_w.detach().double().reshape(m_, 3, 3)
    bo = (out_b.detach().double() if out_b is not None else torch.zeros(n1, dtype=torch.float64, device=out_w.device)).repeat_interleave(mult)
    d = torch.zeros((m_, c, 5, 5), dtype=torch.float64, device=out_w.device)
    cb = torch.zeros((m_,), dtype=torch.float64, device=out_w.device)
    for r in range(3):
        for s_ in range(3):
            if (rmask >> r) & 1 and (smask >> s_) & 1:
                d[:, :, r:r + 3, s_:s_ + 3] += wd[:, r, s_, None, None, None] * wo
                cb += wd[:, r, s_] * bo
    if dw_b is not None:
        cb += dw_b.detach().double()
    wp = pt_w.detach().double().reshape(pt_w.shape[0], m_)
    we = torch.einsum('nm,mcae->naec', wp, d)                            # [N, 5, 5, C]
    const = wp @ cb
    if lat_wk is not None:
        wl = lat_wk.detach().double()                                    # [C, Cin]
        we = torch.cat([we, float(alpha) * torch.einsum('naec,ci->naei', we, wl)], -1)
    return we, const


def _rpn_extra(out_b, dw_w, dw_b, pt_w, scale, shift, lat_wk, alpha):
    others = [t for t in (out_b, dw_w, dw_b, pt_w, scale, shift, lat_wk) if t is not None]
    return tuple(v for t in others for v in (t.data_ptr(), t._version)) + (float(alpha),)


def rpn_composite(out_w, out_b, dw_w, dw_b, pt_w, scale, shift, lat_wk=None, alpha=1.0, parts=None):
    """The RPN's strided reader composed with the output convolution in front of it (evaluation mode): fpn.py:137,145 `out_conv`
    (3x3 / pad 1, linear) -> layers.py:22-29 depthwise 3x3 / stride S / pad 1 (channel multiplier m) -> 1x1 -> BatchNorm (running
    statistics) -> SiLU is ONE 5x5 / stride S / pad 2 convolution of the merged map followed by scale / shift / SiLU:
        W_eff[n][a, e][c] = sum_m pt[n][m] sum_{r + u = a, s + v = e} dw[m][r, s] out_w[m // mult][c][u, v]
        const[n]          = sum_m pt[n][m] (sum_{r, s} dw[m][r, s] out_b[m // mult] + dw_b[m])
    `lat_wk` [C][Cin] (+ alpha): the lateral 1x1 in front of out_conv was deferred, the operands are [up(x1) + b | t] and the weights
    [W_eff | alpha W_eff W_lat].  `scale`, `shift`: `bn_affine` of the block (1x1 bias folded in).  `parts`: channel ranges
    ((c0, c1), ...) of K -- one weight tensor [N][25 * (c1 - c0)] (tap-major) per range, for launches that each take a slice of the
    channels; default: all of K in one.
    -> (tuple of weight tensors, scale [N], shift' [N] = scale * const + shift) for the cells whose nine depthwise taps all lie inside
    the map; float64 arithmetic, once per weight version.  Border cells: `rpn_composite_delta`."""
    def make():
        we, const = _rpn_composite64(out_w, out_b, dw_w, dw_b, pt_w, 7, 7, lat_wk, alpha)
        rng = parts if parts is not None else ((0, we.shape[-1]),)
        ws = tuple(we[..., c0:c1].reshape(we.shape[0], -1).float().contiguous() for c0, c1 in rng)
        return ws, scale, (scale.double() * const + shift.double()).float().contiguous()
    return _cached(out_w, ('rpnc', lat_wk is not None, parts), make, extra=_rpn_extra(out_b, dw_w, dw_b, pt_w, scale, shift, lat_wk, alpha))


def rpn_composite_delta(out_w, out_b, dw_w, dw_b, pt_w, scale, shift, rmask, smask, taps, lat_wk=None, alpha=1.0):
    """Border cells of `rpn_composite`: the depthwise convolution pads the OUTPUT of out_conv with zeros, which a padded 5x5 convolution
    of the input does not reproduce -- a cell whose depthwise tap rows / columns are not all inside the map (`rmask` / `smask`: bit set =
    inside) has weights of its own.  -> (dw [N][len(taps) * K], dshift [N]): scale * (W_class - W_interior) on the listed patch taps
    (a * 5 + e; the caller lists those where the difference is not zero and the patch can hold data) and scale * (const_class -
    const_interior) -- the BatchNorm scale is folded in, so the launch that applies them needs no per-channel epilogue operand."""
    def make():
        we, const = _rpn_composite64(out_w, out_b, dw_w, dw_b, pt_w, rmask, smask, lat_wk, alpha)
        wi, ci = _rpn_composite64(out_w, out_b, dw_w, dw_b, pt_w, 7, 7, lat_wk, alpha)
        d = (we - wi).reshape(we.shape[0], 25, -1)[:, list(taps)] * scale.double()[:, None, None]
        return d.reshape(d.shape[0], -1).float().contiguous(), (scale.double() * (const - ci)).float().contiguous()
    return _cached(out_w, ('rpnd', int(rmask), int(smask), tuple(taps), lat_wk is not None), make,
                   extra=_rpn_extra(out_b, dw_w, dw_b, pt_w, scale, shift, lat_wk, alpha))


XFOLD_COLS = 4      # source columns per cell column that `nbm_cell_patches_up_cols` writes
_XFOLD_GEOM = {}


def xfold_columns(W, Wc, S):
    """The horizontal half of the align-corners bilinear top-down merge (fpn.py:143-144) seen from the cell columns of a 3x3 / stride S /
    pad 1 reader composed with a 3x3 in front of it: the five pixels x = S ox - 2 + l of a patch row read source columns x0(l), x1(l) of
    the Wc-wide coarse map with weights hx, lx -- the fp32 expressions of `cell_input_up_kernel` (fx = sw * clamp(x), x0 = (int) fx,
    x1 = x0 + (x0 < Wc - 1), lx = clamp(fx - x0), hx = 1 - lx), evaluated here in numpy float32.  A pixel outside the image reads
    nothing; x0 == x1 puts both weights on one column.
    -> (xbase int [OW]: the first column any in-image pixel of cell column ox reads; used bool [OW][4]: the window's columns that are
        read; cx float64 [OW][5][4]: pixel l = sum_s cx[ox][l][s] * column xbase[ox] + s), or None when some cell column reads more than
    XFOLD_COLS consecutive columns (a ratio far from 1/2)."""
    import numpy as np
    key = (int(W), int(Wc), int(S))
    if key not in _XFOLD_GEOM:
        OW = (W - 1) // S + 1
        f32 = np.float32
        sw = f32(Wc - 1) / f32(W - 1) if W > 1 else f32(0.0)
        x = S * np.arange(OW)[:, None] - 2 + np.arange(5)[None, :]                      # [OW][5]
        inside = (x >= 0) & (x < W)
        fx = sw * np.clip(x, 0, W - 1).astype(f32)
        assert fx.dtype == np.float32
        x0 = fx.astype(np.int64)
        x1 = x0 + (x0 < Wc - 1)
        lx = np.minimum(np.maximum(fx - x0.astype(f32), f32(0.0)), f32(1.0))
        hx = f32(1.0) - lx
        xbase = np.where(inside, x0, np.iinfo(np.int64).max).min(1)
        hit = None
        if int(np.where(inside, x1 - xbase[:, None], 0).max()) < XFOLD_COLS:
            cx = np.zeros((OW, 5, XFOLD_COLS), dtype=np.float64)
            used = np.zeros((OW, XFOLD_COLS), dtype=bool)
            for ox in range(OW):
                for l in range(5):
                    if inside[ox, l]:
                        cx[ox, l, x0[ox, l] - xbase[ox]] += float(hx[ox, l])
                        cx[ox, l, x1[ox, l] - xbase[ox]] += float(lx[ox, l])
                        used[ox, x0[ox, l] - xbase[ox]] = used[ox, x1[ox, l] - xbase[ox]] = True
            hit = (xbase, used, cx)
        _XFOLD_GEOM[key] = hit
    return _XFOLD_GEOM[key]


def xfold64(we, cx):
    """float64: we [N][R][5][C] (R patch rows of 5 pixels) and cx [G][5][4] of `xfold_columns` ->
    Wf [G][N][R][4][C] = sum_l cx[g][l][s] we[n][r][l][c]: the weights of the window's columns instead of the row's pixels."""
    return torch.einsum('gls,nrlc->gnrsc', cx, we)


def rpn_composite_xfold(out_w, out_b, dw_w, dw_b, pt_w, scale, shift, W, Wc, S, smasks, rows=None, lat_wk=None, alpha=1.0):
    """The interpolated operand's share of `rpn_composite` (channels [0, C) of K: up(x1) + b behind a deferred lateral) with the
    horizontal interpolation folded into the weights, for `nbm_cell_patches_up_cols`' operand: one weight matrix per cell column ox,
    built from the weights of that column's OWN class (`smasks[ox]`: its depthwise tap columns inside the map) -- the left column's
    border difference is in its group's weights.
    rows = None -> [OW][N][20 C] (plane-major K: 4 j + s), the cells whose depthwise tap rows all lie inside the map.
    rows = (rmask, (a, ...)) -> [len(a)][OW][N][4 C]: scale * (W(rmask, smask) - W(7, smask)) on the listed patch rows -- what a row of
    border cells adds to the former (`rpn_composite_delta` for the grouped operand).  float64 arithmetic, once per weight version and
    geometry; None when `xfold_columns` has no window."""
    geom = xfold_columns(W, Wc, S)
    if geom is None:
        return None
    smasks = tuple(int(s) for s in smasks)
    c = out_w.shape[1]

    def make():
        cx = torch.from_numpy(geom[2]).to(out_w.device)
        n = pt_w.shape[0]
        a_rows = list(range(5)) if rows is None else list(rows[1])
        out = torch.empty((len(smasks), n, len(a_rows), XFOLD_COLS * c), dtype=torch.float32, device=out_w.device)
        for sm in sorted(set(smasks)):
            we = _rpn_composite64(out_w, out_b, dw_w, dw_b, pt_w, 7, sm, lat_wk, alpha)[0][..., :c]
            if rows is not None:
                we = (_rpn_composite64(out_w, out_b, dw_w, dw_b, pt_w, rows[0], sm, lat_wk, alpha)[0][..., :c] - we) * \
                    scale.double()[:, None, None, None]
            we = we[:, a_rows]
            oxs = [ox for ox, s in enumerate(smasks) if s == sm]
            for i in range(0, len(oxs), 8):                              # (a float64 copy of the whole result would be 1 GB at 188 x 512)
                sel = torch.tensor(oxs[i:i + 8], device=out_w.device)
                out[sel] = xfold64(we, cx[sel]).reshape(len(sel), n, len(a_rows), -1).float()
        if rows is None:
            return out.reshape(len(smasks), n, -1)
        return out.permute(2, 0, 1, 3).contiguous()
    tag = ('rpnxf', int(W), int(Wc), int(S), smasks, None if rows is None else (int(rows[0]), tuple(rows[1])), lat_wk is not None)
    return _cached(out_w, tag, make, extra=_rpn_extra(out_b, dw_w, dw_b, pt_w, scale, shift, lat_wk, alpha))


def rpn_composite_delta_part(out_w, out_b, dw_w, dw_b, pt_w, scale, shift, rmask, smask, taps, c0, c1, lat_wk=None, alpha=1.0):
    """`rpn_composite_delta` for channels [c0, c1) of K alone: (dw [N][len(taps) * (c1 - c0)], dshift [N])."""
    def make():
        d, dsh = rpn_composite_delta(out_w, out_b, dw_w, dw_b, pt_w, scale, shift, rmask, smask, taps, lat_wk=lat_wk, alpha=alpha)
        d = d.reshape(d.shape[0], len(taps), -1)[:, :, c0:c1]
        return d.reshape(d.shape[0], -1).contiguous(), dsh
    return _cached(out_w, ('rpndp', int(rmask), int(smask), tuple(taps), int(c0), int(c1), lat_wk is not None), make,
                   extra=_rpn_extra(out_b, dw_w, dw_b, pt_w, scale, shift, lat_wk, alpha))


def lateral_of_projection(lat_w, lat_b, proj_w, proj_b):
    """FPN lateral 1x1 (fpn.py:143) applied to `fm + final_projection(ctx)` (self_attention.py:55,76) without forming that sum:
    lateral(fm + W_o ctx + b_o) = W_l fm + (W_l W_o) ctx + (W_l b_o + b_l).  -> (W_l W_o as KRSC rows [N][d], shift [N]); float64
    arithmetic, once per weight version (evaluation mode: fpn.FPN.forward on a `Projected` level)."""
    def make():
        wl = lat_w.detach().double().reshape(lat_w.shape[0], -1)
        wc = wl @ proj_w.detach().double()
        sh = wl @ proj_b.detach().double() + (lat_b.detach().double() if lat_b is not None else 0.0)
        return wc.float().contiguous(), sh.float().contiguous()
    others = [t for t in (lat_b, proj_w, proj_b) if t is not None]
    return _cached(lat_w, 'latproj', make, extra=tuple(v for t in others for v in (t.data_ptr(), t._version)))


def value_of_lateral(lat_w, proj_w, val_w, val_b):
    """The attention's value projection composed with its final projection AND the FPN lateral that reads the level (evaluation mode):
    ctx W_o^T W_l^T = P (x W_v^T + b_v) W_o^T W_l^T = P (x W_v'^T + b_v') with W_v' = W_l W_o W_v [p][C], b_v' = W_l W_o b_v -- the value
    rows are p = 384 wide instead of d = C / 2, and P V' IS the lateral's image of the attention branch (rows of P sum to one).
    -> (W_v' [p][C], b_v' [p]); float64 arithmetic, once per weight version."""
    def make():
        wlo = lat_w.detach().double().reshape(lat_w.shape[0], -1) @ proj_w.detach().double()      # [p][d]
        return (wlo @ val_w.detach().double()).float().contiguous(), (wlo @ val_b.detach().double()).float().contiguous()
    others = [proj_w, val_w, val_b]
    return _cached(lat_w, 'vallat', make, extra=tuple(v for t in others for v in (t.data_ptr(), t._version)))


def pad_attention(ws, Cp, dp):
    """(wq, bq, wk, bk, wv, bv, wo, bo) of a SelfAttention module (C -> d -> C) zero-padded to Cp / dp: [dp, Cp] x 3 with [dp] biases,
    wo [Cp, dp], bo [Cp].  Differentiable (F.pad)."""
    wq, bq, wk, bk, wv, bv, wo, bo = ws
    C_, d = wq.shape[1], wq.shape[0]
    inner = lambda w_, b_: (F.pad(w_, (0, Cp - C_, 0, dp - d)), F.pad(b_, (0, dp - d)))
    return (*inner(wq, bq), *inner(wk, bk), *inner(wv, bv), F.pad(wo, (0, dp - d, 0, Cp - C_)), F.pad(bo, (0, Cp - C_)))


def attention_padded(ws, Cp, dp):
    """`pad_attention` once per weight version (evaluation mode)."""
    extra = tuple(v for t in ws[1:] for v in (t.data_ptr(), t._version))
    return _cached(ws[0], ('attnpad', Cp, dp), lambda: tuple(t.detach().contiguous() for t in pad_attention(ws, Cp, dp)), extra=extra)


def cat_rows(tag, *tensors):
    """Concatenate several [Ni, K] weight matrices (or [Ni] biases) along dim 0, cached on the first."""
    def make():
        return torch.cat([t.detach().reshape(t.shape[0], -1) if t.dim() > 1 else t.detach() for t in tensors], 0).contiguous()
    extra = tuple(v for t in tensors for v in (t.data_ptr(), t._version))
    return _cached(tensors[0], ('cat', tag), make, extra=extra)


def clear():
    _cache.clear()
