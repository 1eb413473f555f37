"""Shared test helpers: oracle-vs-golden plumbing (oracle = checker only) and the random record
filling of the synthetic batches (test_gpu_parity.random_batch, directed_sched.build)."""
import hashlib

import numpy as np

import _oracle
from tiny_mp2v_dec_amd._lib import COEF_DC, COEF_FIRST1S, MB_DCT_FIELD, MB_FIELD_MC, MB_INTRA
from tiny_mp2v_dec_amd.records import Parsed


def oracle_frames(parsed: Parsed):
    """Decode-order frames from the C oracle: list of [Y, U, V] arrays."""
    g, pool = _oracle.reconstruct(parsed.width, parsed.height, parsed.chroma_format, parsed.pics, parsed.mbs,
                                  parsed.coefs, parsed.npics)
    frames = []
    for d in range(parsed.npics):
        base = d * g.slot_bytes
        planes = []
        for p in range(3):
            st, pw, ph = g.stride[p], g.pw[p], g.ph[p]
            arr = pool[base + g.plane_off[p]: base + g.plane_off[p] + st * ph].reshape(ph, st)[:, :pw]
            planes.append(arr.copy())
        frames.append(planes)
    return frames


class SlotOracle:
    """The oracle's pool indexed by slot across batches, with slots that something other than a
    decode filled: preload() puts visible planes into a slot (its padding is left as it is, the
    oracle never reads it), decode() runs a batch on the pool as it stands, grow() adds zero slots."""

    def __init__(self, width, height, cf, nslots):
        self.width, self.height, self.cf, self.nslots = width, height, cf, nslots
        self.g = _oracle.geometry(width, height, cf)
        self.pool = np.zeros(int(self.g.slot_bytes) * nslots + 64, np.uint8)

    def _plane(self, slot, p):
        g, base = self.g, slot * int(self.g.slot_bytes)
        return self.pool[base + g.plane_off[p]: base + g.plane_off[p] + g.stride[p] * g.ph[p]] \
            .reshape(g.ph[p], g.stride[p])[:, :g.pw[p]]

    def planes(self, slot):
        return [self._plane(slot, p) for p in range(3)]

    def preload(self, slot, planes):
        for p in range(3):
            self._plane(slot, p)[:] = planes[p]

    def decode(self, pics, mbs, coefs):
        _oracle.reconstruct(self.width, self.height, self.cf, np.ascontiguousarray(pics), mbs, coefs, self.nslots,
                            pool=self.pool)

    def grow(self, nslots):
        assert nslots >= self.nslots
        pool = np.zeros(int(self.g.slot_bytes) * nslots + 64, np.uint8)
        pool[:int(self.g.slot_bytes) * self.nslots] = self.pool[:int(self.g.slot_bytes) * self.nslots]
        self.pool, self.nslots = pool, nslots


def yuv_md5(planes):
    h = hashlib.md5()
    for p in planes:
        h.update(np.ascontiguousarray(p).tobytes())
    return h.hexdigest()


def _inside(width, height, cf, mbx, mby, mvx, mvy, field, fs):
    pw = [width] + [width if cf == 3 else width // 2] * 2
    ph = [height] + [height if cf != 1 else height // 2] * 2
    for plane in range(3):
        mx, my = mvx, mvy
        if plane:
            if cf < 3:
                mx >>= 1
            if cf < 2:
                my >>= 1
        w = 16 if plane == 0 else (16 if cf == 3 else 8)
        h = 16 if plane == 0 else (8 if cf == 1 else 16)
        x0 = mbx * w + (mx >> 1)
        x1 = x0 + w - 1 + (mx & 1)
        if not field:
            y0 = mby * h + (my >> 1)
            y1 = y0 + h - 1 + (my & 1)
        else:
            y0 = mby * h + fs + 2 * (my >> 1)
            y1 = y0 + 2 * (h // 2 - 1) + 2 * (my & 1)
        if x0 < 0 or y0 < 0 or x1 > pw[plane] - 1 or y1 > ph[plane] - 1:
            return False
    return True


def fill_mb(rng, m, coefs, width, height, cf, all_intra, dirs, field=True, big=False):
    """Fill MB record m (its x, y set) with random content of every record feature and append its
    coefficient words to the list coefs: intra when all_intra (else one in ten), otherwise
    predicted with the direction flags drawn from dirs (one entry: no draw), random vectors kept
    inside the planes, field MC / field DCT, dense residuals (saturating levels with big)."""
    nb = {1: 6, 2: 8, 3: 12}[cf]
    tag = (int(m["x"]) & 7) << 26

    def coef_pack(level, pos, block, flags, _mbx):  # _lib.coef_pack on plain ints
        return (level & 0xFFFF) | (pos << 16) | (block << 22) | flags | tag

    m["qscale"] = rng.integers(1, 113)
    intra = all_intra or rng.random() < 0.1
    flags = 0
    if intra:
        flags |= MB_INTRA
        cbp = (1 << nb) - 1
    else:
        flags |= dirs[rng.integers(0, len(dirs))] if len(dirs) > 1 else dirs[0]
        fld = field and rng.random() < 0.3
        if fld:
            flags |= MB_FIELD_MC
            for r in range(2):
                for s in range(2):
                    if rng.random() < 0.5:
                        flags |= 1 << (8 + 2 * r + s)
        # vectors that keep every read inside every plane
        for r in range(2 if fld else 1):
            for s in range(2):
                for _ in range(20):
                    mx, my = rng.integers(-40, 40), rng.integers(-40, 40)
                    if _inside(width, height, cf, m["x"], m["y"], mx, my, fld, (flags >> (8 + 2 * r + s)) & 1):
                        break
                else:
                    mx, my = 0, 0
                    if fld:
                        flags &= ~(1 << (8 + 2 * r + s))
                        flags |= r << (8 + 2 * r + s)
                m["mv"][r, s] = (mx, my)
        cbp = int(rng.integers(0, 1 << nb)) if rng.random() < 0.7 else 0
    if cbp and rng.random() < 0.4 and cf != 3:  # 4:4:4 field DCT is refused (test_validate.py)
        flags |= MB_DCT_FIELD
    m["flags"], m["cbp"] = flags, cbp
    m["coef_off"] = len(coefs)
    for b in range(nb):
        if not cbp >> b & 1:
            continue
        pos = 0
        if intra:
            coefs.append(coef_pack(int(rng.integers(0, 2048)), 0, b, COEF_DC, m["x"]))
            pos = 1
        elif rng.random() < 0.3:
            coefs.append(coef_pack(int(rng.choice([-1, 1])), 0, b, COEF_FIRST1S, m["x"]))
            pos = 1
        ncoef = int(rng.integers(0 if intra else 1, 20))
        for _ in range(ncoef):
            pos += int(rng.integers(0, 4))
            if pos > 63:
                break
            lvl = int(rng.integers(-2048, 2048)) if (big and rng.random() < 0.3) else int(rng.integers(-40, 41))
            coefs.append(coef_pack(lvl, pos, b, 0, m["x"]))
            pos += 1
    m["ncoef"] = len(coefs) - m["coef_off"]
