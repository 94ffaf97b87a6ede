"""NumPy statement of the common corruptions: THE definition of dvd_corrupt_rgb8 and ops.corrupt_rgb8, byte for
byte.  Integer arithmetic throughout; the real-valued tables (Poisson CDFs, FIR weights) are read from the library's host export
dvd_corrupt_table, and `reference_table` restates them in float64 NumPy for the test that holds the export to one quantum.

Formats: Philox4x32-10 with counter (element index in the image, draw, kind, 0 = element noise | 1 = image parameter) and key
(seed & 0xffffffff, crc32(path)); Q16 gains and FIR weights; Q8 zoom coordinates and bilinear fractions; a Q8 channel mean."""
import ctypes as C
import zlib

import numpy as np

NAMES = ("gaussian_noise", "shot_noise", "impulse_noise", "defocus_blur", "glass_blur", "motion_blur", "zoom_blur", "snow", "frost",
         "fog", "brightness", "contrast", "elastic_transform", "pixelate", "jpeg_compression", "speckle_noise", "gaussian_blur",
         "spatter", "saturate")
KERNEL_KINDS = (0, 1, 2, 3, 5, 6, 10, 11, 13, 15, 16)      # dvd_corrupt_rgb8
DELIVERED = KERNEL_KINDS + (14,)                          # 14: the JPEG codec
REFUSED = (4, 7, 8, 9, 12, 17, 18)
FIR_KINDS = (3, 5, 16)

SIGMA_MILLI = (80, 120, 180, 260, 380)
SPECKLE = (15, 20, 35, 45, 60)
IMPULSE = (3, 6, 9, 17, 27)
PHOTONS = (60, 25, 12, 5, 3)
DEFOCUS = ((3, .1), (4, .5), (6, .5), (8, .5), (10, .5))
MOTION = ((10, 3), (15, 5), (15, 8), (15, 12), (20, 15))
GAUSS_SIGMA = (1, 2, 3, 4, 6)
ZOOM = ((1, 111), (1, 116), (2, 121), (2, 126), (3, 133))   # step and end of the zoom, in hundredths
LIFT = (26, 51, 76, 102, 128)                               # np.rint(255 * c), c = .1 .. .5
KEEP = (40, 30, 20, 10, 5)
CELLS = (60, 50, 40, 30, 25)
JPEG_QUALITY = (25, 18, 15, 10, 7)
MIN_SIDE, MAX_SIDE = 32, 16384

U32 = np.uint64(0xffffffff)


def key(seed, path):
    return (int(seed) & 0xffffffff, zlib.crc32(str(path).encode()))


def philox(k0, k1, c0, c1, c2, c3):
    """Philox4x32-10 on arrays (uint64 holding 32-bit values): four words."""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & U32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & U32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & U32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & U32, (k1 + np.uint64(0xBB67AE85)) & U32
    return c0, c1, c2, c3


def irwin_hall(k, n):
    """z * 2^16 of elements 0..n-1: twelve 16-bit uniforms (draw 0: four words, draw 1: two) minus 6 * 65535."""
    e = np.arange(n, dtype=np.uint64)
    a, b = philox(*k, e, 0, 0, 0), philox(*k, e, 1, 0, 0)
    s = sum((v & np.uint64(0xffff)) + (v >> np.uint64(16)) for v in (*a, b[0], b[1]))
    return s.astype(np.int64) - 6 * 65535


def table(kind, severity, angle=0):
    """The library's own table (dvd_corrupt_table): kind 1 [256, c] thresholds, FIR kinds [side, side] Q16 weights."""
    from dvd_amd import lib
    raw = lib.raw()
    n = raw.dvd_corrupt_table(kind, severity, angle, None, 0)
    assert n > 0, (kind, severity, n)
    buf = (C.c_uint32 * n)()
    assert raw.dvd_corrupt_table(kind, severity, angle, buf, n) == n
    t = np.frombuffer(buf, np.uint32).astype(np.int64)
    if kind == 1:
        return t.reshape(256, PHOTONS[severity - 1])
    side = int(round(n ** 0.5))
    return t.reshape(side, side)


def fir_real(kind, severity, angle=0):
    """The FIR weights in float64 before quantisation, normalised to sum 1."""
    s = severity - 1
    if kind == 16:
        r = 4 * GAUSS_SIGMA[s]
        y, x = np.mgrid[-r:r + 1, -r:r + 1]
        wt = np.exp(-(x * x + y * y) / (2.0 * GAUSS_SIGMA[s] ** 2))
    elif kind == 3:
        rd, alias = DEFOCUS[s]
        g = 2 if rd > 8 else 1
        r = rd + g
        gw = np.exp(-np.arange(-g, g + 1) ** 2 / (2.0 * alias * alias))
        gw /= gw.sum()
        wt = np.zeros((2 * r + 1, 2 * r + 1))
        for dy in range(-rd, rd + 1):
            for dx in range(-rd, rd + 1):
                if dx * dx + dy * dy <= rd * rd:
                    wt[dy + r - g:dy + r + g + 1, dx + r - g:dx + r + g + 1] += np.outer(gw, gw)
    else:
        r, sigma = MOTION[s]
        wt = np.zeros((2 * r + 1, 2 * r + 1))
        th = angle * np.pi / 180.0
        for i in range(-r, r + 1):
            gi = np.exp(-(i * i) / (2.0 * sigma * sigma))
            fx, fy = i * np.cos(th), i * np.sin(th)
            x0, y0 = int(np.floor(fx)), int(np.floor(fy))
            ax, ay = fx - x0, fy - y0
            for k, wk in enumerate(((1 - ay) * (1 - ax), (1 - ay) * ax, ay * (1 - ax), ay * ax)):
                x, y = x0 + (k & 1), y0 + (k >> 1)
                if wk > 0 and -r <= x <= r and -r <= y <= r:
                    wt[y + r, x + r] += gi * wk
    return wt / wt.sum()


def reference_table(kind, severity, angle=0):
    """float64 NumPy restatement of dvd_corrupt_table."""
    if kind == 1:
        c = PHOTONS[severity - 1]
        out = np.zeros((256, c), np.int64)
        for x in range(256):
            lam = x * c / 255.0
            p, cdf = np.exp(-lam), 0.0
            for j in range(c):
                if j:
                    p = p * lam / j
                cdf += p
                out[x, j] = min(int(np.floor(cdf * 4294967296.0)), 0xffffffff)
        return out
    wt = fir_real(kind, severity, angle)
    q = np.rint(wt * 65536.0).astype(np.int64)
    q.flat[int(np.argmax(q))] += 65536 - int(q.sum())
    return q


def motion_angle(k):
    return int(philox(*k, 0, 0, 5, 1)[0]) % 91 - 45


def reflect101(i, n):
    i = np.where(i < 0, -i, np.where(i > n - 1, 2 * (n - 1) - i, i))
    return np.clip(i, 0, n - 1)


def fir(img, wt):
    """Q16 weights [side, side] over a reflect-101 border, 32-bit accumulation, (acc + 32768) >> 16."""
    h, w = img.shape[:2]
    r = wt.shape[0] // 2
    pad = img[reflect101(np.arange(-r, h + r), h)][:, reflect101(np.arange(-r, w + r), w)].astype(np.int64)
    acc = np.zeros(img.shape, np.int64)
    for dy in range(wt.shape[0]):
        for dx in range(wt.shape[1]):
            if wt[dy, dx]:
                acc += int(wt[dy, dx]) * pad[dy:dy + h, dx:dx + w]
    assert acc.max() < 2 ** 32
    return ((acc + 32768) >> 16).astype(np.uint8)


def zoom_coord(x, n, zc):
    return (((n - 1) * (zc - 100) + 200 * x) << 7) // zc


def zoom(img, severity):
    h, w = img.shape[:2]
    step, end = ZOOM[severity - 1]
    p = img.astype(np.int64)
    acc = p << 16
    zooms = list(range(100, end, step))
    for zc in zooms:
        cy, cx = zoom_coord(np.arange(h), h, zc), zoom_coord(np.arange(w), w, zc)
        y0, x0, ay, ax = cy >> 8, cx >> 8, (cy & 255)[:, None, None], (cx & 255)[None, :, None]
        y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
        acc += (256 - ay) * ((256 - ax) * p[y0][:, x0] + ax * p[y0][:, x1]) + ay * ((256 - ax) * p[y1][:, x0] + ax * p[y1][:, x1])
    den = (len(zooms) + 1) << 16
    return ((acc + den // 2) // den).astype(np.uint8)


def brightness(img, severity):
    p = img.astype(np.int64)
    v = p.max(axis=2, keepdims=True)
    v2 = np.minimum(v + LIFT[severity - 1], 255)
    scaled = (2 * p * v2 + v) // np.maximum(2 * v, 1)
    return np.where(v == 0, v2, scaled).astype(np.uint8)


def contrast(img, severity):
    h, w = img.shape[:2]
    keep = (KEEP[severity - 1] * 65536 + 50) // 100
    p = img.astype(np.int64)
    mean8 = (p.sum(axis=(0, 1)) * 256 + (h * w) // 2) // (h * w)
    return np.clip((mean8 * (65536 - keep) + p * 256 * keep + (1 << 23)) >> 24, 0, 255).astype(np.uint8)


def pixelate_cells(n, severity):
    """(m, cell index of every output position) along one axis of n pixels."""
    m = n * CELLS[severity - 1] // 100
    return m, ((2 * np.arange(n) + 1) * m) // (2 * n)


def _overlaps(n, m):
    s, i = np.arange(n)[None, :], np.arange(m)[:, None]
    return np.maximum(np.minimum((s + 1) * m, (i + 1) * n) - np.maximum(s * m, i * n), 0)      # [m, n], rows sum to n


def pixelate(img, severity):
    h, w = img.shape[:2]
    (mh, iy), (mw, ix) = pixelate_cells(h, severity), pixelate_cells(w, severity)
    rows = np.tensordot(_overlaps(h, mh), img.astype(np.int64), axes=(1, 0))                       # [mh, w, 3]
    acc = np.tensordot(rows, _overlaps(w, mw), axes=(1, 1)).transpose(0, 2, 1)                     # [mh, mw, 3]
    small = (acc + (h * w) // 2) // (h * w)
    return small[iy][:, ix].astype(np.uint8)


def jpeg(img, severity):
    import jpeg_model as J
    import jpegdec_model as M
    return M.decode(J.model_file(img, JPEG_QUALITY[severity - 1], "420"))[0]


def corrupt(img, kind, severity, k):
    """One image [h, w, 3] uint8 -> the corrupted image.  k = (k0, k1)."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape[:2]
    assert kind in DELIVERED and 1 <= severity <= 5 and min(h, w) >= MIN_SIDE and max(h, w) <= MAX_SIDE
    s = severity - 1
    x = img.reshape(-1).astype(np.int64)
    if kind == 0:
        gain = (255 * SIGMA_MILLI[s] * 65536 + 500) // 1000
        out = np.clip(x + ((gain * irwin_hall(k, x.size) + (1 << 31)) >> 32), 0, 255)
    elif kind == 15:
        gain = (SPECKLE[s] * 65536 + 50) // 100
        out = np.clip(x + ((x * gain * irwin_hall(k, x.size) + (1 << 31)) >> 32), 0, 255)
    elif kind == 2:
        u = philox(*k, np.arange(x.size, dtype=np.uint64), 0, 2, 0)[0].astype(np.int64)
        t_lo, t_hi = (IMPULSE[s] << 32) // 100, (IMPULSE[s] << 32) // 200
        out = np.where(u < t_hi, 255, np.where(u < t_lo, 0, x))
    elif kind == 1:
        u = philox(*k, np.arange(x.size, dtype=np.uint64), 0, 1, 0)[0].astype(np.int64)
        c = PHOTONS[s]
        t = table(1, severity)
        count = sum((t[:, j][x] < u).astype(np.int64) for j in range(c))
        out = (2 * 255 * count + c) // (2 * c)
    elif kind in FIR_KINDS:
        return fir(img, table(kind, severity, motion_angle(k) if kind == 5 else 0))
    elif kind == 6:
        return zoom(img, severity)
    elif kind == 10:
        return brightness(img, severity)
    elif kind == 11:
        return contrast(img, severity)
    elif kind == 13:
        return pixelate(img, severity)
    else:
        return jpeg(img, severity)
    return out.astype(np.uint8).reshape(img.shape)


def sample_image(h, w, seed=0):
    """A page-like picture with every byte value, flat areas, edges and a black and a white patch."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([(x * 255) // (w - 1), (y * 255) // (h - 1), ((x + y) * 7) % 256], axis=2).astype(np.uint8)
    img[h // 4:h // 2, w // 4:w // 2] = rng.randint(0, 256, (h // 2 - h // 4, w // 2 - w // 4, 3))
    img[:6, :9] = 0
    img[-7:, -5:] = 255
    img[h // 2:h // 2 + 5, :w // 3] = (200, 30, 90)
    return img
