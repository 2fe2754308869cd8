"""Training forward + backward of the transformer head (`--tf_rcnn`) with and without dropout (csrc/dropout.hip, csrc/mha.hip); writes
profiles/tf_dropout.txt and prints one JSON line.

    python scripts/bench_tf_dropout.py [--batch 128] [--rois 16] [--layers 6] [--ps 0,0.1] [--rounds 7] [--window_ms 200]
                                       [--parent parent.json] [--out profiles/tf_dropout.txt]

One process builds a head per (encoder flavour, p) on the same weights and inputs and times `forward_nhwc` in training mode plus the
backward pass of a linear loss: HIP events around windows of about --window_ms of back-to-back steps after a warm-up, --rounds
windows per variant, the variants alternating; median, minimum and maximum per step.  The p = 0 head issues the launches it issued
before dropout existed, so its figure is the one to compare with the same line of the parent commit: `--ps 0 --out ''` runs on
that commit too, and `--parent` quotes the JSON line such a run printed."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from bench_resnext import stats, timed          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--rois', type=int, default=16)
    ap.add_argument('--layers', type=int, default=6)
    ap.add_argument('--ps', default='0,0.1')
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--window_ms', type=float, default=200.0)
    ap.add_argument('--parent', default='')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tf_dropout.txt'))
    a = ap.parse_args()
    import torch
    from birdsoundclassif_amd import synth
    from birdsoundclassif_amd.nets.layers import Transformer_RCNN
    from birdsoundclassif_amd.train import default_args
    assert torch.cuda.is_available(), 'this benchmark needs the GPU: there is no CPU path'
    B, R, C = a.batch, a.rois, 256
    ps = [float(p) for p in a.ps.split(',')]
    gen = torch.Generator(device='cuda')
    gen.manual_seed(5)
    pool = torch.randn(B * R, 2, 2, C, generator=gen, device='cuda').abs()
    pe = torch.randn(B * R, 2, 2, C, generator=gen, device='cuda')
    r1, r2 = torch.randn(B * R, 604, generator=gen, device='cuda'), torch.randn(B * R, 151, generator=gen, device='cuda')
    n = torch.full((1,), R, dtype=torch.int32, device='cuda')
    rows = []
    for pe_qk in (False, True):
        windows = {}
        for p in ps:
            head = Transformer_RCNN(default_args(device='cuda', tf_rcnn=True, tf_pe_qk=pe_qk, tf_num_encoder_layers=a.layers, dropout=p))
            sd = synth.fill_state_dict({k: tuple(v.shape) for k, v in head.state_dict().items()})
            head.load_state_dict(sd)
            head = head.cuda().train()
            if p > 0:
                head.set_dropout_stream(1234, 0)

            def step(head=head):
                head.zero_grad(set_to_none=True)
                x = pool.detach().requires_grad_(True)
                reg, cls = head.forward_nhwc(x, pe, B, R, n)
                ((reg * r1).sum() + (cls * r2).sum()).backward()

            windows[p] = timed(step, a.rounds, a.window_ms)
        ms = {p: [] for p in ps}
        for _ in range(a.rounds):
            for p in ps:                                   # the variants alternate
                ms[p].append(windows[p][0]())
        for p in ps:
            rows.append(dict(flavour='tf_pe_qk' if pe_qk else 'default', p=p, steps_per_window=windows[p][1], **stats(ms[p])))
    result = dict(bench='tf_dropout', batch=B, rois=R, layers=a.layers, tokens=B * R, device=torch.cuda.get_device_name(0), rows=rows)
    if a.out:
        parent = json.loads(open(a.parent).read().strip().splitlines()[-1]) if a.parent else None
        with open(a.out, 'w') as f:
            f.write(f'Transformer head, training forward + backward, B = {B}, {R} RoIs ({B * R} tokens of 512 floats), {a.layers} encoder '
                    f'layers, {result["device"]}\n')
            f.write(f'HIP events around windows of ~{a.window_ms:.0f} ms of back-to-back steps, {a.rounds} windows per variant, variants '
                    'alternating in one process (scripts/bench_tf_dropout.py)\n\n')
            f.write(f'{"flavour":10s} {"p":>5s} {"median us":>10s} {"min us":>10s} {"max us":>10s} {"steps/window":>13s}\n')
            for r in rows:
                f.write(f'{r["flavour"]:10s} {r["p"]:5.2f} {r["median_us"]:10.1f} {r["min_us"]:10.1f} {r["max_us"]:10.1f} '
                        f'{r["steps_per_window"]:13d}\n')
            f.write('\nNo threshold is set on these numbers.  With p = 0.1 a layer runs three more element-wise launches forward and '
                    'three backward, its two residual additions leave the GEMM epilogues for them, and the attention kernels evaluate '
                    'Philox4x32-10 once per probability.\n')
            if parent is not None:
                f.write('\nParent commit, same command in a process of its own in the same session (where its launches are the same the '
                        'figures should agree within the spread shown):\n')
                for r in parent['rows']:
                    f.write(f'{r["flavour"]:10s} {r["p"]:5.2f} {r["median_us"]:10.1f} {r["min_us"]:10.1f} {r["max_us"]:10.1f} '
                            f'{r["steps_per_window"]:13d}\n')
            else:
                f.write('\nParent commit at p = 0: not measured in this run.\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
