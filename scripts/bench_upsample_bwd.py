"""The general bilinear-backward kernel (`upsample_bwd_kernel`, csrc/pointwise_bwd.hip) of this tree's library against another build of
the same ABI, both loaded in ONE process, the runs alternating (profiles/pointwise_edges.txt).

    python scripts/bench_upsample_bwd.py --parent /path/to/other/libnbm_hip.so [--shape 94,256,235,640,64] [--batch 8] [--rounds 15] [--inner 20]

HIP events around `--inner` back-to-back launches, `--rounds` windows per library, the order swapped every round; median, minimum and
maximum per launch, and whether the two results have the same bits."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', required=True)
    ap.add_argument('--shape', default='94,256,235,640,64', help='Hi,Wi,Ho,Wo,C')
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--inner', type=int, default=20)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'this benchmark needs the GPU: there is no CPU path'
    libs = {'new': C.CDLL(os.path.join(ROOT, 'birdsoundclassif_amd', 'libnbm_hip.so')), 'parent': C.CDLL(os.path.abspath(a.parent))}
    for lib in libs.values():
        lib.nbm_upsample_bilinear_bwd.restype = C.c_int
        lib.nbm_upsample_bilinear_bwd.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    Hi, Wi, Ho, Wo, Cc = (int(v) for v in a.shape.split(','))
    B = a.batch
    torch.manual_seed(0)
    gy = torch.randn(B, Ho, Wo, Cc, device='cuda')
    outs = {k: torch.empty(B, Hi, Wi, Cc, device='cuda') for k in libs}

    def run(k):
        rc = libs[k].nbm_upsample_bilinear_bwd(gy.data_ptr(), B, Hi, Wi, Cc, outs[k].data_ptr(), Ho, Wo, 0, None)
        assert rc == 0, rc

    for k in libs:
        for _ in range(3):
            run(k)
    torch.cuda.synchronize()
    times = {k: [] for k in libs}
    for r in range(a.rounds):
        for k in (('new', 'parent') if r % 2 == 0 else ('parent', 'new')):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                run(k)
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / a.inner * 1000)
    print(f'({Hi},{Wi}) -> ({Ho},{Wo}), C = {Cc}, B = {B}: '
          + ', '.join(f'{k} median {statistics.median(v):.1f} us (min {min(v):.1f}, max {max(v):.1f})' for k, v in times.items())
          + f'; bit-equal {torch.equal(outs["new"], outs["parent"])}, max |new - parent| {float((outs["new"] - outs["parent"]).abs().max()):.3g}')


if __name__ == '__main__':
    main()
