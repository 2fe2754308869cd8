"""The proposal chain (top-N selection + greedy NMS) at pre-NMS budgets up to the whole map; prints a table and one JSON line.

    python scripts/bench_proposals.py [--rounds 7] [--window_ms 60] [--skip_detect]

Seeded RPN outputs on the 24 x 64 map (23 040 anchors) are decoded once; `ops.rpn_select` + `ops.nms_batched` are then timed
with HIP events around windows of about --window_ms of back-to-back calls after a warm-up, --rounds windows per variant, the
variants of one batch alternating (a drift of the clock hits all alike); median, minimum and maximum per call.

* B = 64 with the evaluation counts (post_n 50, every image a segment of its own) and B = 128 with the training counts
  (post_n 1 000, one segment);
* pre = 3 000 on the small route (the control), pre = 4 096 on the small route and on the forced big route (the only size both
  take), pre = 6 000, 12 000 and 23 040 on the big route;
* the NMS alone on 23 040 disjoint boxes per image with post_n = cap: the walk without an early stop;
* the whole eager detect step (B = 64, filler weights) at --pre_nms_topN_eval 6 000 against the default 500."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KA, FAIL_BELOW, NMS_THRESH = 23040, 16, 0.7


def timed(fn, window_ms):
    """-> a closure that times one window of back-to-back calls (its length chosen from a first timed call) in ms per call."""
    import torch
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(), fn(), e1.record()
    torch.cuda.synchronize()
    reps = max(3, min(2000, int(window_ms / max(e0.elapsed_time(e1), 1e-3))))

    def window():
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps
    return window, reps


def stats(ms, reps):
    return {'median_us': round(1e3 * statistics.median(ms), 1), 'min_us': round(1e3 * min(ms), 1), 'max_us': round(1e3 * max(ms), 1),
            'reps': reps}


def alternate(variants, rounds, window_ms):
    """{name: fn} -> {name: stats}, the windows of the variants alternating."""
    windows = {name: timed(fn, window_ms) for name, fn in variants.items()}
    ms = {name: [] for name in variants}
    for _ in range(rounds):
        for name, (window, _) in windows.items():
            ms[name].append(window())
    return {name: stats(ms[name], windows[name][1]) for name in variants}


def decoded(B, seed):
    """Seeded RPN outputs of B images (softmaxed class pairs, deltas) through nbm_rpn_decode -> boxes, keys, kept counts."""
    import torch
    from birdsoundclassif_amd import ops
    from birdsoundclassif_amd.nets.layers import ProposalLayer
    from birdsoundclassif_amd.train import default_args
    gen = torch.Generator(device='cuda')
    gen.manual_seed(seed)
    cls = (1.5 * torch.randn(B, 24, 64, 15, 2, generator=gen, device='cuda')).softmax(-1).reshape(B, 24, 64, 30)
    reg = 0.25 * torch.randn(B, 24, 64, 60, generator=gen, device='cuda')
    anchors = ProposalLayer(default_args(), 5).anchors(24, 64, 'cuda')
    assert anchors.shape[0] == KA
    return ops.rpn_decode(cls, reg, anchors, 15, 1024, 375, 5)


def chain_leg(B, post_n, coupled, rounds, window_ms):
    import torch
    from birdsoundclassif_amd import ops
    boxes, keys, cnt = decoded(B, B)
    seg = ops.batch_segments(B, None if coupled else 1)
    variants, info = {}, {}
    for name, pre, force in (('pre 3000 small', 3000, False), ('pre 4096 small', 4096, False), ('pre 4096 big (forced)', 4096, True),
                             ('pre 6000 big', 6000, False), ('pre 12000 big', 12000, False), ('pre 23040 big', 23040, False)):
        top_n, cap, route = ops.proposal_plan(pre, KA)
        assert (route == 'big') == (cap > 4096)

        def chain(top_n=top_n, cap=cap, force=force):
            sb, ss, n_sel = ops.rpn_select(boxes, keys, cnt, top_n, FAIL_BELOW, cap, segments=seg, force_big=force)
            return ops.nms_batched(sb, ss, n_sel, NMS_THRESH, post_n, segments=seg, force_big=force)
        variants[name] = chain
        info[name] = {'top_n': top_n, 'cap': cap, 'n_out': sorted(set(chain()[2].tolist()))}
    a, b = variants['pre 4096 small'](), variants['pre 4096 big (forced)']()
    assert all(torch.equal(x, y) for x, y in zip(a, b)), 'the two routes differ at 4096'
    # the walk without an early stop: 23 040 disjoint boxes per image, every one kept
    cap = 32768
    x = 20.0 * torch.arange(cap, device='cuda', dtype=torch.float32)
    dis = torch.stack([x, torch.zeros_like(x), x + 9, torch.full_like(x, 9.0)], 1)[None].expand(B, -1, -1).contiguous()
    dis_scores = torch.rand(B, cap, device='cuda')
    n_in = torch.full((B,), KA, device='cuda', dtype=torch.int32)
    variants['nms only, 23040 disjoint, post_n = cap'] = lambda: ops.nms_batched(dis, dis_scores, n_in, NMS_THRESH, cap, segments=seg)
    assert variants['nms only, 23040 disjoint, post_n = cap']()[2].tolist() == [KA] * B
    info['nms only, 23040 disjoint, post_n = cap'] = {'top_n': KA, 'cap': cap, 'n_out': [KA]}
    res = alternate(variants, rounds, window_ms)
    for name in res:
        res[name].update(info[name])
    return res


def detect_leg(B, rounds):
    import torch
    from birdsoundclassif_amd import synth
    from birdsoundclassif_amd.nets import build_model
    from birdsoundclassif_amd.train import default_args
    gen = torch.Generator(device='cuda')
    gen.manual_seed(1)
    imgs = torch.rand(B, 1, 375, 1024, generator=gen, device='cuda')
    variants, keepalive = {}, []
    for pre in (500, 6000):
        model, _ = build_model(default_args(device='cuda', pre_nms_topN_eval=pre))
        model.load_state_dict(synth.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}))
        model = model.cuda().eval()
        keepalive.append(model)
        variants[f'detect step, pre_nms_topN_eval {pre}'] = lambda model=model: model.detect(imgs, 0.3, 0.05, independent=True)
    with torch.no_grad():
        return alternate(variants, rounds, 400.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--window_ms', type=float, default=60.0)
    ap.add_argument('--skip_detect', action='store_true')
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'bench_proposals.py measures on the GPU; there is nothing to report without one'
    res = {'bench': 'proposals', 'rounds': a.rounds, 'window_ms': a.window_ms, 'KA': KA, 'nms_thresh': NMS_THRESH}
    with torch.no_grad():
        res['B64_eval_post50'] = chain_leg(64, 50, False, a.rounds, a.window_ms)
        res['B128_train_post1000'] = chain_leg(128, 1000, True, a.rounds, a.window_ms)
    if not a.skip_detect:
        res['B64_detect_step'] = detect_leg(64, a.rounds)
    for leg in ('B64_eval_post50', 'B128_train_post1000', 'B64_detect_step'):
        if leg in res:
            print(leg)
            for name, s in res[leg].items():
                print(f'  {name:42s} median {s["median_us"]:11.1f} us   min {s["min_us"]:11.1f}   max {s["max_us"]:11.1f}   '
                      f'reps {s["reps"]:5d}' + (f'   cap {s["cap"]:6d}  n_out {s["n_out"]}' if 'cap' in s else ''))
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
