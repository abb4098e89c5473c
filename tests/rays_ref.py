"""Independent restatement of the ray-batch contract in numpy:
Philox4x32-10 and the picks in integers, the directions elementwise in
fp32 / fp64 (elementwise numpy operations do not fuse)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF

# Random123 known answers: (counter, key) -> output
KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(ctr, key):
    """ctr: four uint64 arrays (or ints) holding 32-bit words; key: two ints.
    Returns four uint64 arrays of 32-bit words."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK) for v in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(MASK)]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def words(seed, step, i, stream):
    """key = (seed lo, seed hi), counter = (i, step lo, step hi, stream)."""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    return philox4x32_10((i, step & MASK, step >> 32, stream), (seed & MASK, seed >> 32))


def mulhi(word, n):
    return ((np.asarray(word, dtype=np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def batch_draw(seed, step, F, H, W, S=None):
    """Once per batch (stream 1, i = 0): patch origin, white?, drawn frame."""
    r = [int(v) for v in words(seed, step, 0, 1)]
    origin = None if S is None else (int(mulhi(r[0], W - S + 1)), int(mulhi(r[1], H - S + 1)))
    return origin, r[2] >= 2 ** 31, int(mulhi(r[3], F))


def picks(mode, seed, step, H, W, S=None):
    """(px, py) int64 [R] of a batch, in ray order."""
    if mode == "random":
        r = words(seed, step, np.arange(S * S, dtype=np.uint64), 0)
        return mulhi(r[0], W), mulhi(r[1], H)
    if mode == "patch":
        (ox, oy), _, _ = batch_draw(seed, step, 1, H, W, S)
        i = np.arange(S * S, dtype=np.int64)
        return ox + i % S, oy + i // S
    i = np.arange(H * W, dtype=np.int64)
    return i % W, i // W


def cam_row(campos, camrot, K):
    """One row of the device camera table, fp32 [16]."""
    K = np.asarray(K)
    return np.concatenate([np.asarray(camrot, np.float32).reshape(9), np.asarray(campos, np.float32).reshape(3),
                           np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]]).astype(np.float32)])


def focal_K(focal, H, W):
    return np.array([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1]], np.float64)


def directions64(px, py, cam, dir_norm=False):
    """[R,3] fp64 before the one rounding: x, y in three fp32 operations each,
    the rotation in fp64 on the widened fp32 values, left to right."""
    cam = np.asarray(cam, np.float32)
    px, py = np.asarray(px, np.float32), np.asarray(py, np.float32)
    half = np.float32(0.5)
    x = ((px + half) - cam[14]) / cam[12]
    y = ((py + half) - cam[15]) / cam[13]
    assert x.dtype == np.float32 and y.dtype == np.float32
    x, y = x.astype(np.float64), y.astype(np.float64)
    R = cam[:9].astype(np.float64).reshape(3, 3)
    d = np.stack([(x * R[i, 0] + y * R[i, 1]) + R[i, 2] for i in range(3)], -1)
    if dir_norm:
        n = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        d = d / (n + 1e-5)[:, None]
    return d


def directions(px, py, cam, dir_norm=False):
    return directions64(px, py, cam, dir_norm).astype(np.float32)


def ulp_distance(a, b):
    """Elementwise distance of two fp32 arrays in units in the last place."""
    def order(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(order(a) - order(b))
