"""The transformer head in the DETR flavour (`--tf_rcnn --tf_pe_qk`) beyond 128 RoIs per image -- the long attention kernels of
csrc/mha.hip -- and a control at the sizes the short kernels serve; writes profiles/tf_long.txt and prints one JSON line.

    python scripts/bench_tf_long.py [--parent_root DIR] [--alt_root DIR] [--alternations 3] [--layers 6] [--rounds 7] [--window_ms 150]
                                    [--out profiles/tf_long.txt]

Every measurement runs in a child process of its own (`--section`), so the control can alternate between two trees: this one and
`--parent_root`, a built tree of the parent commit -- the default flavour at 8 heads, training forward + backward at B = 128 / 16 RoIs
and evaluation at B = 64 / 50 RoIs (the sizes of scripts/bench_tf_head_dims.py), `--alternations` times each, this tree first.  The
launches are the same in both trees; the figures should agree within the spread between the processes of one tree.

New range, `tf_pe_qk`, d_model 512, 8 heads (head dim 64): evaluation at B = 64 with 129, 200, 300 and 1 024 RoIs; training forward +
backward at B = 128 with 160 and 256 RoIs, p = 0 and 0.1.  Per row: the head's step, the attention launches alone on operands of the
same geometry times the layer count, the same attention as float32 torch (bmm, softmax, bmm and autograd's backward; dropout through
torch's own generator) as an outside yardstick, and for training the peak memory of one attention backward (its workspace).
`--alt_root`: a second built tree of this commit whose library was compiled with another block shape (csrc/mha.hip,
`-DMHA_LROWS=4`: blocks of 16 query rows, one workgroup per CU); its new-range rows are measured after this tree's, in a process of
their own, and written as section 3.
HIP events around windows of about --window_ms of back-to-back steps after a warm-up, --rounds windows per figure; median, minimum,
maximum."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTROL_TRAIN, CONTROL_EVAL = (128, 16), (64, 50)        # (images, RoIs per image)
EVAL_B, EVAL_ROIS = 64, (129, 200, 300, 1024)
TRAIN_B, TRAIN_ROIS, TRAIN_PS = 128, (160, 256), (0.0, 0.1)
E, NHEAD = 512, 8


def section(a):
    """One child process: measure `a.section` with the package of `a.root`."""
    sys.path.insert(0, os.path.join(HERE, 'scripts'))
    from bench_resnext import stats, timed          # (puts this tree in front of the path: the section's tree goes back in front)
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    import birdsoundclassif_amd
    from birdsoundclassif_amd import _lib, ops, synth
    assert os.path.abspath(birdsoundclassif_amd.__file__).startswith(os.path.abspath(a.root) + os.sep), birdsoundclassif_amd.__file__
    from birdsoundclassif_amd.nets.layers import Transformer_RCNN
    from birdsoundclassif_amd.train import default_args
    assert torch.cuda.is_available(), 'this benchmark needs the GPU: there is no CPU path'
    gen = torch.Generator(device='cuda')
    gen.manual_seed(5)
    randn = lambda *s: torch.randn(*s, generator=gen, device='cuda')

    def measure(fn):
        window, reps = timed(fn, a.rounds, a.window_ms)
        return dict(steps_per_window=reps, **stats([window() for _ in range(a.rounds)]))

    def head_step(pe_qk, B, R, p, train):
        head = Transformer_RCNN(default_args(device='cuda', tf_rcnn=True, tf_pe_qk=pe_qk, tf_num_encoder_layers=a.layers, dropout=p,
                                             tf_model_dim=E, tf_nhead=NHEAD))
        head.load_state_dict(synth.fill_state_dict({k: tuple(v.shape) for k, v in head.state_dict().items()}))
        head = head.cuda().train(train)
        if train and p > 0:
            head.set_dropout_stream(1234, 0)
        pool, pe, r1, r2 = randn(B * R, 2, 2, 256).abs(), randn(B * R, 2, 2, 256), randn(B * R, 604), randn(B * R, 151)
        n = torch.full((1,), R, dtype=torch.int32, device='cuda')

        def step():
            head.zero_grad(set_to_none=True)
            x = pool.detach().requires_grad_(True)
            reg, cls = head.forward_nhwc(x, pe, B, R, n)
            ((reg * r1).sum() + (cls * r2).sum()).backward()

        def infer():
            with torch.no_grad():
                head.forward_nhwc(pool, pe, B, R, n)

        return step if train else infer

    def attention(pe_qk, B, R, p, train):
        """-> (the attention launches of one layer, the backward alone or None) on random operands of the head's geometry."""
        geom = (R, B, NHEAD, 1, R) if pe_qk else (B, R, NHEAD, R, 1)
        qkv, go = randn(B * R, 3 * E), randn(B * R, E)
        q, k, v = qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:]
        n = torch.full((1,), R, dtype=torch.int32, device='cuda') if pe_qk else None
        if not train:
            return (lambda: ops.mha_small(q, k, v, *geom, n)), None
        if p > 0:
            bwd = lambda: ops.mha_small_drop_bwd(q, k, v, go, *geom, n, p, 1234, 0, 0)
            return (lambda: (ops.mha_small_drop(q, k, v, *geom, n, p, 1234, 0, 0), bwd())), bwd
        bwd = lambda: ops.mha_small_bwd(q, k, v, go, *geom, n)
        return (lambda: (ops.mha_small(q, k, v, *geom, n), bwd())), bwd

    def torch_attention(B, R, p, train):
        """float32 torch on the same GPU: [B * NHEAD, R, hd] operands, bmm + softmax + bmm (+ dropout, + autograd's backward)."""
        hd = E // NHEAD
        q, k, v = (randn(B * NHEAD, R, hd).requires_grad_(train) for _ in range(3))
        go = randn(B * NHEAD, R, hd)

        def fwd():
            prob = torch.softmax(torch.bmm(q, k.transpose(1, 2)) * hd ** -0.5, -1)
            if train and p > 0:
                prob = torch.nn.functional.dropout(prob, p)
            return torch.bmm(prob, v)

        if not train:
            def run():
                with torch.no_grad():
                    fwd()
            return run

        def run():
            q.grad = k.grad = v.grad = None
            fwd().backward(go)
        return run

    rows = []
    if a.section == 'control':
        for (B, R), train in ((CONTROL_TRAIN, True), (CONTROL_EVAL, False)):
            whole = measure(head_step(False, B, R, 0.0, train))
            att = measure(attention(False, B, R, 0.0, train)[0])
            rows.append(dict(mode='train p=0.00' if train else 'eval', batch=B, rois=R, **whole,
                             attention_us=round(att['median_us'] * a.layers, 1)))
    else:
        cases = [(EVAL_B, R, 0.0, False) for R in EVAL_ROIS] + [(TRAIN_B, R, p, True) for R in TRAIN_ROIS for p in TRAIN_PS]
        if a.only:
            cases = [c for i, c in enumerate(cases) if str(i) in a.only.split(',')]
        for B, R, p, train in cases:
            whole = measure(head_step(True, B, R, p, train))
            both, bwd = attention(True, B, R, p, train)
            att = measure(both)
            yard = measure(torch_attention(B, R, p, train))
            row = dict(mode=f'train p={p:.2f}' if train else 'eval', batch=B, rois=R, **whole,
                       attention_us=round(att['median_us'] * a.layers, 1), attention_min_us=round(att['min_us'] * a.layers, 1),
                       attention_max_us=round(att['max_us'] * a.layers, 1),
                       attention_share=round(att['median_us'] * a.layers / whole['median_us'], 3),
                       torch_attention_us=round(yard['median_us'] * a.layers, 1),
                       plan=ops.mha_plan(R, E // NHEAD, B, NHEAD)._asdict())
            if bwd is not None:
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                bwd()
                torch.cuda.synchronize()
                row['backward_peak_bytes'] = torch.cuda.max_memory_allocated() - base
            rows.append(row)
            torch.cuda.empty_cache()
    print(json.dumps(dict(section=a.section, root=a.root, library=_lib.LIB_PATH, device=torch.cuda.get_device_name(0), rows=rows)))


def child(a, sec, root, extra=()):
    cmd = [sys.executable, os.path.abspath(__file__), '--section', sec, '--root', root, '--layers', str(a.layers), '--rounds', str(a.rounds),
           '--window_ms', str(a.window_ms), *extra]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=a.child_timeout).stdout
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent_root', default='')
    ap.add_argument('--alt_root', default='', help='a built tree with another long-kernel block shape: its new-range rows become section 3')
    ap.add_argument('--alternations', type=int, default=3)
    ap.add_argument('--layers', type=int, default=6)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--window_ms', type=float, default=150.0)
    ap.add_argument('--child_timeout', type=float, default=400.0)
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'tf_long.txt'))
    ap.add_argument('--section', default='', help='internal: control | new')
    ap.add_argument('--root', default=HERE, help='internal: the tree whose package a section imports')
    ap.add_argument('--only', default='', help='new range: comma-separated case indices (0-3 evaluation, 4-7 training)')
    a = ap.parse_args()
    if a.section:
        return section(a)
    control = []
    for i in range(a.alternations):
        control.append(('this', child(a, 'control', HERE)))
        if a.parent_root:
            control.append(('parent', child(a, 'control', os.path.abspath(a.parent_root))))
    new = child(a, 'new', HERE, ('--only', a.only) if a.only else ())
    alt = child(a, 'new', os.path.abspath(a.alt_root), ('--only', a.only) if a.only else ()) if a.alt_root else None
    result = dict(bench='tf_long', layers=a.layers, device=new['device'], control=[dict(tree=t, rows=r['rows']) for t, r in control],
                  rows=new['rows'], alt_rows=alt['rows'] if alt else None)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(f'Transformer head alone, {a.layers} encoder layers, d_model {E}, {NHEAD} heads, {result["device"]}\n')
            f.write(f'HIP events around windows of ~{a.window_ms:.0f} ms of back-to-back steps, {a.rounds} windows per figure, a process per '
                    'section (scripts/bench_tf_long.py)\n\n')
            f.write(f'1. Control, default flavour (short kernels): training forward + backward at B = {CONTROL_TRAIN[0]} / {CONTROL_TRAIN[1]} '
                    f'RoIs, evaluation at B = {CONTROL_EVAL[0]} / {CONTROL_EVAL[1]} RoIs; processes in the order run\n')
            f.write(f'{"tree":7s} {"mode":13s} {"median us":>10s} {"min us":>10s} {"max us":>10s} {"attention us":>13s}\n')
            for t, r in control:
                for row in r['rows']:
                    f.write(f'{t:7s} {row["mode"]:13s} {row["median_us"]:10.1f} {row["min_us"]:10.1f} {row["max_us"]:10.1f} '
                            f'{row["attention_us"]:13.1f}\n')
            if not a.parent_root:
                f.write('parent commit: not measured in this run\n')
            def table(rows):
                f.write(f'{"mode":13s} {"B":>4s} {"RoIs":>5s} {"median us":>11s} {"min us":>11s} {"max us":>11s} {"attention us":>13s} {"share":>6s} '
                        f'{"torch us":>11s} {"x torch":>8s} {"bwd peak MiB":>13s}\n')
                for r in rows:
                    peak = f'{r["backward_peak_bytes"] / 2 ** 20:13.1f}' if 'backward_peak_bytes' in r else f'{"-":>13s}'
                    f.write(f'{r["mode"]:13s} {r["batch"]:4d} {r["rois"]:5d} {r["median_us"]:11.1f} {r["min_us"]:11.1f} {r["max_us"]:11.1f} '
                            f'{r["attention_us"]:13.1f} {r["attention_share"]:6.1%} {r["torch_attention_us"]:11.1f} '
                            f'{r["attention_us"] / r["torch_attention_us"]:8.2f} {peak}\n')

            shape = lambda rows: f'{rows[0]["plan"]["rows"]} query rows and {rows[0]["plan"]["lds_bytes"]} B of LDS per workgroup'
            f.write(f'\n2. New range, tf_pe_qk (long kernels; head dim 64; {shape(new["rows"])}).  attention us: the attention launches alone x '
                    'layers; share: of the median; torch us: the same attention as float32 torch bmm + softmax + bmm on the same GPU x layers\n')
            table(new['rows'])
            if alt:
                f.write(f'\n3. The same rows on the library of --alt_root ({shape(alt["rows"])})\n')
                table(alt['rows'])
            f.write('\nbwd peak: peak allocation of one attention backward above its operands -- the workspace of 8 * B * heads * S * S bytes '
                    'and the three gradients.  No threshold is set on the numbers of section 2.\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
