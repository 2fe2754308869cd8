"""CPU reference and input generators for the per-file merge tests (tests/test_merge_cpu.py, tests/test_gpu_long_recordings.py).

`greedy_keep` is the greedy NMS of `oracle.nets_ref.greedy_nms_keep` (walk in the given order, a kept box removes every later
box with IoU >= thresh) in numpy fp32 with the operation order of `oracle.nets_ref.pair_iou`, but it only evaluates the
candidates whose x-range can overlap the kept box, so it scales to the 2^17 boxes of the device kernel's limit."""
import numpy as np

ONE, ZERO = np.float32(1), np.float32(0)
HOP, W_PIX = 819, 1024


def iou_f32(a, b):
    """pair_iou for box a [4] against boxes b [m,4], float32, same association order (+1 pixel, union = (aa + ab) - inter)."""
    xi = np.maximum((np.minimum(a[2], b[:, 2]) - np.maximum(a[0], b[:, 0])) + ONE, ZERO)
    yi = np.maximum((np.minimum(a[3], b[:, 3]) - np.maximum(a[1], b[:, 1])) + ONE, ZERO)
    inter = xi * yi
    aa = ((a[2] - a[0]) + ONE) * ((a[3] - a[1]) + ONE)
    ab = ((b[:, 2] - b[:, 0]) + ONE) * ((b[:, 3] - b[:, 1]) + ONE)
    return inter / ((aa + ab) - inter)


def greedy_keep(boxes, thresh=0.3):
    """boxes [n,4] (finite) -> list of kept indices in walk order.  A pair whose x-ranges are more than 2 apart has a
    non-positive x overlap in fp32 too (the operations are monotone), hence IoU 0 < thresh: only the others are evaluated."""
    assert thresh > 0
    b = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 4)
    n = len(b)
    if n == 0:
        return []
    t = np.float32(thresh)
    order = np.argsort(b[:, 0], kind='stable')
    xs = b[order, 0].astype(np.float64)
    maxw = float((b[:, 2].astype(np.float64) - b[:, 0].astype(np.float64)).max())
    dead = np.zeros(n, dtype=bool)
    keep = []
    for i in range(n):
        if dead[i]:
            continue
        keep.append(i)
        lo = np.searchsorted(xs, float(b[i, 0]) - max(maxw, 0.0) - 2.0, 'left')
        hi = np.searchsorted(xs, float(b[i, 2]) + 2.0, 'right')
        c = order[lo:hi]
        c = c[c > i]
        c = c[~dead[c]]
        if len(c):
            dead[c[iou_f32(b[i], b[c]) >= t]] = True
    return keep


# ----------------------------------------------------------------------------------------------- generators
def ulp_pairs():
    """Three pairs (a, b) at x ~ 1e6 whose fp32 IoU is float32(0.3) minus one ulp, exactly float32(0.3), plus one ulp."""
    t = np.float32(0.3)
    targets = (np.nextafter(t, ZERO), t, np.nextafter(t, ONE))
    X = np.float32(1.0e6)
    a = np.array([X, 10, X + 99, 109], np.float32)
    ys = np.unique((np.float32(11.5) + np.arange(0, 600000) * 1e-6).astype(np.float32))
    B = np.stack([np.full_like(ys, X + 53), ys, np.full_like(ys, X + 152), ys + np.float32(99)], 1)
    v = iou_f32(a, B)
    out = []
    for q in targets:
        hit = np.flatnonzero(v == q)
        assert len(hit), 'no pair found for an ulp target'
        out.append((a.copy(), B[hit[0]].copy()))
    return out


def chain(x):
    """A kills B (IoU 0.43), B would kill C (0.43), A does not reach C (0.11): C survives B's removal."""
    return np.array([[x, 0, x + 99, 99], [x + 40, 0, x + 139, 99], [x + 80, 0, x + 179, 99]], np.float32)


def realistic(n, rng):
    """Detector-like file: 50 integer boxes per 1024-column window, windows 819 columns apart, classes 1..150, class-major
    order (class, window, row) as the collect step emits it."""
    if n == 0:
        return np.zeros((0, 4), np.float32)
    n_win = (n + 49) // 50
    cls = rng.integers(1, 151, size=(n_win, 50))
    x1 = rng.integers(0, 1000, size=(n_win, 50))
    w = rng.integers(5, 400, size=(n_win, 50))
    y1 = rng.integers(0, 300, size=(n_win, 50))
    h = rng.integers(5, 75, size=(n_win, 50))
    x2 = np.minimum(x1 + w, 1023)
    y2 = np.minimum(y1 + h, 374)
    shift = (np.arange(n_win) * HOP)[:, None]
    boxes = np.stack([x1 + shift, y1, x2 + shift, y2], -1).astype(np.float32).reshape(-1, 4)
    key = cls.reshape(-1).astype(np.int64) * n_win + np.repeat(np.arange(n_win), 50)
    return boxes[np.argsort(key, kind='stable')][:n]


def dense(n, rng):
    """Every box overlaps every other one (one region at x ~ 1e6, fractional coordinates), with runs of identical boxes."""
    x1 = np.float32(1.0e6) + rng.uniform(0, 200, n).astype(np.float32)
    y1 = rng.uniform(0, 100, n).astype(np.float32)
    b = np.stack([x1, y1, x1 + rng.uniform(300, 800, n).astype(np.float32), y1 + rng.uniform(150, 270, n).astype(np.float32)], 1)
    b = b.astype(np.float32)
    for s in range(0, n - 3, 97):
        b[s + 1:s + 3] = b[s]
    return b


def scattered(n, rng):
    """Random boxes over a whole-night x range with fractional coordinates (fp32 rounding at 1e6 matters)."""
    x1 = rng.uniform(0, 1.1e6, n).astype(np.float32)
    y1 = rng.uniform(0, 300, n).astype(np.float32)
    w = rng.uniform(1, 1000, n).astype(np.float32)
    h = rng.uniform(1, 75, n).astype(np.float32)
    return np.stack([x1, y1, x1 + w, y1 + h], 1).astype(np.float32)


def with_specials(b):
    """Plant the ulp pairs at the head of the walk and 3-box chains across 64-box block boundaries."""
    b = b.copy()
    n = len(b)
    k = 0
    for j, (p, q) in enumerate(ulp_pairs()):
        if k + 2 > n:
            break
        off = np.float32(5000 * j)
        b[k], b[k + 1] = p + [off, 0, off, 0], q + [off, 0, off, 0]
        k += 2
    for s, x in ((63, 2.0e5), (127, 4.0e5), (4095, 6.0e5), (8191, 8.0e5)):
        if s + 3 <= n:
            b[s:s + 3] = chain(np.float32(x))
    return b


LAYOUTS = {'realistic': realistic, 'dense': dense, 'scattered': scattered}


def make_boxes(layout, n, seed=0):
    return with_specials(LAYOUTS[layout](n, np.random.default_rng(seed)))
