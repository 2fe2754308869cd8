"""The transformer head (`--tf_rcnn`) at head counts on either side of the 64-column limit of the narrow attention kernels
(csrc/mha.hip): training forward + backward with and without dropout, evaluation, and the attention kernels' share of each; writes
profiles/tf_head_dims.txt and prints one JSON line.

    python scripts/bench_tf_head_dims.py [--heads 8,4,2,1] [--layers 6] [--ps 0,0.1] [--rounds 7] [--window_ms 150]
                                         [--parent parent.json] [--out profiles/tf_head_dims.txt]

Geometry of scripts/bench_tf_dropout.py: the head alone, 6 encoder layers, B = 128 / 16 RoIs for training and B = 64 / 50 RoIs for
evaluation; the default flavour at every head count of --heads (d_model 512: head dims 64, 128, 256, 512) and `tf_pe_qk` at
`--tf_model_dim 1024 --tf_nhead 8` (head dim 128).  HIP events around windows of about --window_ms of back-to-back steps after a
warm-up, --rounds windows per variant; median, minimum and maximum per step.  "attention" is the same measurement of the layer's
attention launches alone (forward, and the two backward passes when training) on operands of the same geometry, times the layer count.
At 8 heads the launches are those of the parent commit: `--heads 8 --out ''` runs there too, and `--parent` quotes the JSON line such a
run printed."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from bench_resnext import stats, timed          # noqa: E402

TRAIN, EVAL = (128, 16), (64, 50)               # (images, RoIs per image)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--heads', default='8,4,2,1')
    ap.add_argument('--pe_qk', type=int, default=1, help='0: leave the tf_pe_qk row out (a commit that refuses its head dim)')
    ap.add_argument('--layers', type=int, default=6)
    ap.add_argument('--ps', default='0,0.1')
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--window_ms', type=float, default=150.0)
    ap.add_argument('--parent', default='')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tf_head_dims.txt'))
    a = ap.parse_args()
    import torch
    from birdsoundclassif_amd import ops, synth
    from birdsoundclassif_amd.nets.layers import Transformer_RCNN
    from birdsoundclassif_amd.train import default_args
    assert torch.cuda.is_available(), 'this benchmark needs the GPU: there is no CPU path'
    ps = [float(p) for p in a.ps.split(',')]
    gen = torch.Generator(device='cuda')
    gen.manual_seed(5)
    randn = lambda *s: torch.randn(*s, generator=gen, device='cuda')
    data = {}
    for B, R in (TRAIN, EVAL):
        data[B, R] = (randn(B * R, 2, 2, 256).abs(), randn(B * R, 2, 2, 256), randn(B * R, 604), randn(B * R, 151),
                      torch.full((1,), R, dtype=torch.int32, device='cuda'))
    variants = [dict(tf_pe_qk=False, tf_model_dim=512, tf_nhead=int(h)) for h in a.heads.split(',')]
    if a.pe_qk:
        variants.append(dict(tf_pe_qk=True, tf_model_dim=1024, tf_nhead=8))

    def measure(fn):
        window, reps = timed(fn, a.rounds, a.window_ms)
        return dict(steps_per_window=reps, **stats([window() for _ in range(a.rounds)]))

    def attention(kw, B, R, p, train):
        """The attention launches of one layer on random operands of the head's geometry."""
        E, nh = kw['tf_model_dim'], kw['tf_nhead']
        geom = (R, B, nh, 1, R) if kw['tf_pe_qk'] else (B, R, nh, R, 1)
        qkv, go = randn(B * R, 3 * E), randn(B * R, E)
        q, k, v = qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:]
        n = data[B, R][4] if kw['tf_pe_qk'] else None
        if not train:
            return lambda: ops.mha_small(q, k, v, *geom, n)
        if p > 0:
            return lambda: (ops.mha_small_drop(q, k, v, *geom, n, p, 1234, 0, 0), ops.mha_small_drop_bwd(q, k, v, go, *geom, n, p, 1234, 0, 0))
        return lambda: (ops.mha_small(q, k, v, *geom, n), ops.mha_small_bwd(q, k, v, go, *geom, n))

    rows = []
    for kw in variants:
        name = dict(flavour='tf_pe_qk' if kw['tf_pe_qk'] else 'default', nhead=kw['tf_nhead'], hd=kw['tf_model_dim'] // kw['tf_nhead'])
        for p in ps + [None]:                              # None: evaluation
            train = p is not None
            B, R = TRAIN if train else EVAL
            pool, pe, r1, r2, n = data[B, R]
            head = Transformer_RCNN(default_args(device='cuda', tf_rcnn=True, tf_num_encoder_layers=a.layers, dropout=p or 0, **kw))
            head.load_state_dict(synth.fill_state_dict({k: tuple(v.shape) for k, v in head.state_dict().items()}))
            head = head.cuda().train(train)
            if train and p > 0:
                head.set_dropout_stream(1234, 0)

            def step():
                head.zero_grad(set_to_none=True)
                x = pool.detach().requires_grad_(True)
                reg, cls = head.forward_nhwc(x, pe, B, R, n)
                ((reg * r1).sum() + (cls * r2).sum()).backward()

            def infer():
                with torch.no_grad():
                    head.forward_nhwc(pool, pe, B, R, n)

            whole = measure(step if train else infer)
            att = measure(attention(kw, B, R, p or 0, train))
            rows.append(dict(**name, mode=f'train p={p:.2f}' if train else 'eval', batch=B, rois=R, **whole,
                             attention_us=round(att['median_us'] * a.layers, 1),
                             attention_share=round(att['median_us'] * a.layers / whole['median_us'], 3)))
    result = dict(bench='tf_head_dims', layers=a.layers, device=torch.cuda.get_device_name(0), rows=rows)
    if a.out:
        parent = json.loads(open(a.parent).read().strip().splitlines()[-1]) if a.parent else None
        head_line = (f'{"flavour":9s} {"nhead":>5s} {"hd":>4s} {"mode":13s} {"median us":>10s} {"min us":>10s} {"max us":>10s} '
                     f'{"attention us":>13s} {"share":>6s}\n')
        line = lambda r: (f'{r["flavour"]:9s} {r["nhead"]:5d} {r["hd"]:4d} {r["mode"]:13s} {r["median_us"]:10.1f} {r["min_us"]:10.1f} '
                          f'{r["max_us"]:10.1f} {r["attention_us"]:13.1f} {r["attention_share"]:6.1%}\n')
        with open(a.out, 'w') as f:
            f.write(f'Transformer head alone, {a.layers} encoder layers, {result["device"]}: training forward + backward at B = {TRAIN[0]} / '
                    f'{TRAIN[1]} RoIs, evaluation at B = {EVAL[0]} / {EVAL[1]} RoIs\n')
            f.write(f'HIP events around windows of ~{a.window_ms:.0f} ms of back-to-back steps, {a.rounds} windows per row, one process '
                    '(scripts/bench_tf_head_dims.py)\n')
            f.write('attention us: the attention launches alone on operands of the same geometry, x layers; share: of the median\n\n')
            f.write(head_line)
            for r in rows:
                f.write(line(r))
            f.write('\nNo threshold is set on these numbers.  hd <= 64 runs the narrow kernels (K and V of an (entry, head) whole in LDS); '
                    'above it the wide kernels stage the head dimension in 64-column chunks with a second grid dimension over blocks of 32 '
                    'query rows.  The shape with one workgroup per (entry, head) and no row blocks was not built.\n')
            if parent is not None:
                f.write('\nParent commit, `--heads 8 --pe_qk 0` in a process of its own in the same session (the same launches: the figures '
                        'should agree within the spread shown):\n')
                f.write(head_line)
                for r in parent['rows']:
                    f.write(line(r))
            else:
                f.write('\nParent commit at 8 heads: not measured in this run.\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
