"""NumPy statement of the token -> group maps of nbm_mha_segments (include/nbm_hip.h): which key rows each query row of a
segmented batch attends to.  Token (image b, RoI slot r) is row b * R + r; `table` is the int32 [2, B] segment table
(`ops.segment_table`: first image and image count of every image's segment), `n_roi` one RoI count per image, equal within a
segment.  Rows that do not appear in the map are no tokens: the kernel writes zeros there."""
import numpy as np

ACROSS_ROIS, ACROSS_IMAGES = 0, 1


def token_groups(mode, table, n_roi, R):
    """-> {query row: [key rows, ascending]} over the valid tokens."""
    first, count = np.asarray(table)
    n_roi = np.asarray(n_roi)
    B = len(first)
    b = np.repeat(np.arange(B), R)
    r = np.tile(np.arange(R), B)
    n = np.minimum(n_roi[b] if mode == ACROSS_ROIS else n_roi[first[b]], R)
    out = {}
    for row in np.flatnonzero(r < n):
        bi, ri = int(b[row]), int(r[row])
        if mode == ACROSS_ROIS:
            out[int(row)] = [bi * R + j for j in range(int(n[row]))]
        else:
            out[int(row)] = [(int(first[bi]) + j) * R + ri for j in range(int(count[bi]))]
    return out


def token_groups_per_call(mode, sizes, seg_counts, R):
    """The same map by enumeration of the model calls: segment i (sizes[i] images, seg_counts[i] RoIs per image) is one
    call of the reference on its images alone; inside a call of k images, token (i, r) with r < n attends to the RoIs
    (i, j < n) of its image (ACROSS_ROIS) or to the slot r of every image (j, r), j < k (ACROSS_IMAGES)."""
    out, s = {}, 0
    for k, n in zip(sizes, seg_counts):
        n = min(int(n), R)
        for i in range(k):
            for r in range(n):
                keys = [(i, j) for j in range(n)] if mode == ACROSS_ROIS else [(j, r) for j in range(k)]
                out[(s + i) * R + r] = [(s + a) * R + c for a, c in keys]
        s += k
    return out


def image_counts(sizes, seg_counts):
    """Per-segment RoI counts -> one count per image."""
    return np.repeat(np.asarray(seg_counts, dtype=np.int32), np.asarray(sizes))


def table_of(sizes):
    first = np.repeat(np.cumsum([0] + list(sizes[:-1])), sizes)
    return np.stack([first, np.repeat(sizes, sizes)]).astype(np.int32)


def attention_f64(q, k, v, groups, nhead):
    """float64 softmax attention over the groups: q, k, v [rows, E] -> out [rows, E], zero where a row is no token."""
    q, k, v = (np.asarray(t, dtype=np.float64) for t in (q, k, v))
    rows, E = q.shape
    hd = E // nhead
    out = np.zeros((rows, E))
    for row, keys in groups.items():
        qh = q[row].reshape(nhead, hd)
        kh = k[keys].reshape(len(keys), nhead, hd)
        vh = v[keys].reshape(len(keys), nhead, hd)
        s = np.einsum('hd,jhd->hj', qh, kh) / np.sqrt(hd)
        p = np.exp(s - s.max(1, keepdims=True))
        p /= p.sum(1, keepdims=True)
        out[row] = np.einsum('hj,jhd->hd', p, vh).reshape(E)
    return out
