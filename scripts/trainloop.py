"""Wall time per training step the way bench.py's train leg measures it (no synchronisation inside the loop), alternating blocks
of steps with a module switch on / off:  python trainloop.py B steps_per_block blocks module.SWITCH [module.SWITCH ...]
e.g. `trainloop.py 128 4 3 functional.LAZY_DGRAD`.  Prints the mean step time of every block."""
import sys, os, time, importlib, torch, numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from birdsoundclassif_amd import synth
from birdsoundclassif_amd.nets import build_model
from birdsoundclassif_amd.train import default_args, build_optimizer, train_one_step
B, per, blocks = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
switches = []
for name in sys.argv[4:]:
    mod, attr = name.rsplit('.', 1)
    try:
        m = importlib.import_module('birdsoundclassif_amd.nets.' + mod)
    except ImportError:
        m = importlib.import_module('birdsoundclassif_amd.' + mod)
    switches.append((m, attr, getattr(m, attr)))
args = default_args(device='cuda')
model, crit = build_model(args)
model.load_state_dict(synth.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}))
model = model.cuda().train(); crit.train()
opt, _ = build_optimizer(model, args)
base = synth.image_batch(0, 8)
img = torch.from_numpy(np.tile(base, (-(-B // 8), 1, 1))[:B].copy()).cuda()
bbs, idss, lens = [], [], []
for i in range(B):
    bb, ids, l = synth.label_batch(i % 8, 1); bbs.append(bb); idss.append(ids); lens += l
batch = [img, img, torch.cat(bbs), torch.cat(idss), lens]
np.random.seed(0)
def run(n):
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(n):
        train_one_step(model, crit, opt, batch, args.clip_max_norm, 'cuda', negative_sample=False)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t) / n
for on in (True, False):                       # warm both variants up (allocator, caches)
    for m, a, v in switches:
        setattr(m, a, v if on else (not v if isinstance(v, bool) else 0))
    run(2)
for blk in range(blocks):
    for on in (True, False):
        for m, a, v in switches:
            setattr(m, a, v if on else (not v if isinstance(v, bool) else 0))
        print(f'block {blk} switches {"default" if on else "flipped"}: {run(per):.1f} ms / step', flush=True)
        if not switches:
            break
