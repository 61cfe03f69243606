"""Numpy restatement of vv_obs_synth's generator (include/vaevar.h): Philox4x32-10 in uint64 arithmetic, the mask as a
stable argsort of (key32 << 32) | p, eps with the device's formula evaluated in fp64 on the same bits, and the
selection on arbitrary keys. Nothing here comes from the device."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
STREAM_MASK, STREAM_NOISE = 1, 2


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Counter words (arrays or scalars) and key words -> the four output words, uint32 arrays."""
    c = [np.atleast_1d(np.asarray(x, np.uint64)) & MASK32 for x in (c0, c1, c2, c3)]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    m0, m1, s32 = np.uint64(M0), np.uint64(M1), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]  # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & MASK32, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def _key(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32


def key32(seed, draw, hw):
    p = np.arange(hw, dtype=np.uint64)
    return philox4x32_10(p, 0, STREAM_MASK, int(draw) & 0xFFFFFFFF, *_key(seed))[0]


def select_ref(keys, k):
    """(mask fp32, threshold ties): 1.0 at the k entries smallest in (key, position)."""
    keys = np.asarray(keys).astype(np.uint32)
    n = keys.size
    order = np.argsort((keys.astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64), kind="stable")
    mask = np.zeros(n, np.float32)
    mask[order[:k]] = 1.0
    ties = int((keys == keys[order[k - 1]]).sum()) if k > 0 else 0
    return mask, ties


def mask_ref(seed, draw, hs, ws, n_obs):
    m, ties = select_ref(key32(seed, draw, hs * ws), n_obs)
    return m.reshape(hs, ws), ties


def eps_ref(seed, draw, first, n):
    """eps(first .. first + n - 1) in fp64 from the same bits: u1, u2 exact, then sqrt(-2 ln u1) cos / sin(2 pi u2)."""
    e = np.arange(first, first + n, dtype=np.uint64)
    g = e >> np.uint64(2)
    lane = (e & np.uint64(3)).astype(np.int64)
    w = philox4x32_10(g & MASK32, g >> np.uint64(32), STREAM_NOISE, int(draw) & 0xFFFFFFFF, *_key(seed))
    wa = np.where(lane < 2, w[0], w[2]).astype(np.uint64)
    wb = np.where(lane < 2, w[1], w[3]).astype(np.uint64)
    u1 = ((wa >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (wb >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    ang = 2.0 * np.pi * u2
    return np.where(lane % 2 == 0, r * np.cos(ang), r * np.sin(ang))
