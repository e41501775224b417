"""A seeded writer of legal GRAY and LUT-based ICC profiles for tests/test_color_link_plan.py and the GPU tests: lut8 (mft1),
lut16 (mft2) and lutAToB (mAB) elements under A2B0, XYZ and Lab connection space, version 2 and 4.  The tables describe a
plausible device: a gamma, a colourant matrix (Adobe RGB's or Display P3's, D50), and a mild twist of the linear light that is
zero at the cube's corners.  Every profile comes with the stages it holds as arrays (LutProfile.stages), for the f64 statement
the builder is checked against."""
import struct

import numpy as np

from tests import color_profile_emulation as E

D50 = np.array([0.9642, 1.0, 0.8249])
MAX_XYZ = 1.0 + 32767.0 / 32768.0
P3_XYZ = ((0.5151, 0.2412, -0.0011), (0.2919, 0.6922, 0.0419), (0.1572, 0.0666, 0.7841))      # colourants of R, G, B (D50)


class Device:
    def __init__(self, seed):
        rng = np.random.RandomState(seed)
        self.gamma = float(rng.choice([1.8, 2.0, 2.2, 2.4]))
        mix = rng.uniform(0.0, 1.0)
        m = mix * np.array(E.ADOBE_XYZ).T + (1 - mix) * np.array(P3_XYZ).T       # rows X, Y, Z; columns R, G, B
        self.m = m * (D50 / m.sum(axis=1))[:, None]                               # device white is the PCS's white
        self.twist = float(rng.uniform(0.03, 0.08))

    def twisted(self, lin):
        """linear light [..., 3] -> the device's linear light with its twist, still inside 0..1"""
        lin = np.asarray(lin, np.float64)
        r, g, b = lin[..., 0], lin[..., 1], lin[..., 2]
        t = self.twist
        return np.clip(np.stack([r + t * r * (1 - r) * (g - b), g + t * g * (1 - g) * (b - r), b + t * b * (1 - b) * (r - g)], axis=-1), 0.0, 1.0)

    def xyz(self, lin):
        return self.twisted(lin) @ self.m.T


def lab_from_xyz(xyz):
    t = np.asarray(xyz, np.float64) / D50
    f = np.where(t > (24 / 116) ** 3, np.cbrt(np.maximum(t, 0)), (841 / 108) * t + 16 / 116)
    return np.stack([116 * f[..., 1] - 16, 500 * (f[..., 0] - f[..., 1]), 200 * (f[..., 1] - f[..., 2])], axis=-1)


def encode_pcs(xyz, pcs, how):
    """XYZ [..., 3] -> uint16 [..., 3] in the encoding `how`: "16v2" (lut16), "8" (lut8, widened x 257), "v4" (mAB)"""
    if pcs == b"XYZ ":
        v = np.clip(np.asarray(xyz) / MAX_XYZ, 0, 1)
        return np.round(v * (255 if how == "8" else 65535)).astype(np.uint16) * (257 if how == "8" else 1)
    lab = lab_from_xyz(xyz)
    unit = np.stack([lab[..., 0] / 100, (lab[..., 1] + 128) / 255, (lab[..., 2] + 128) / 255], axis=-1)
    scale = {"16v2": 65280, "8": 255, "v4": 65535}[how]
    return np.round(np.clip(unit, 0, 1) * scale).clip(0, 65535 if how != "8" else 255).astype(np.uint16) * (257 if how == "8" else 1)


class LutProfile:
    def __init__(self, name, icc, stages, pcs, version, element):
        self.name, self.icc, self.stages, self.pcs, self.version, self.element = name, icc, stages, pcs, version, element

    def __repr__(self):
        return self.name


def _grid_points(grid):
    axes = [np.arange(g) / (g - 1) for g in grid]
    return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1)                   # [g0, g1, g2, 3] = r, g, b


def _power_table(n, exponent):
    return np.round((np.arange(n) / (n - 1)) ** exponent * 65535).astype(np.uint16)


def mft_profile(seed, wide=True, pcs=b"XYZ ", version=2, grid=9, in_entries=256, out_entries=256):
    """lut8 (wide=False: 256-entry tables of bytes) or lut16.  Input tables: the device's gamma (2 entries: the identity, the CLUT
    takes the gamma); output tables: x^1.25 over a CLUT that stores the 1/1.25 power (2 entries: the identity)."""
    dev = Device(seed)
    if not wide:
        in_entries = out_entries = 256
    pre = 1.0 if in_entries == 2 else (dev.gamma if pcs == b"XYZ " else dev.gamma / 2.0)     # Lab: half the gamma ahead of the CLUT
    post = 1.0 if out_entries == 2 or pcs != b"XYZ " else 1.25
    how = "16v2" if wide else "8"
    clut = encode_pcs(dev.xyz(_grid_points((grid,) * 3) ** (dev.gamma / pre)), pcs, how)
    if post != 1.0:
        clut = np.round((clut / 65535.0) ** (1 / post) * 65535).astype(np.uint16)
    tin, tout = _power_table(in_entries, pre), _power_table(out_entries, post)
    if not wide:
        tin, tout, clut = (tin >> 8) * 257, (tout >> 8) * 257, (clut >> 8) * 257
    put = (lambda a: b"".join(struct.pack(">H", int(v)) for v in a.ravel())) if wide else (lambda a: bytes(int(v) >> 8 for v in a.ravel()))
    ident = b"".join(E.s15(v) for v in (1, 0, 0, 0, 1, 0, 0, 0, 1))
    elem = (b"mft2" if wide else b"mft1") + b"\0" * 4 + bytes([3, 3, grid, 0]) + ident
    if wide:
        elem += struct.pack(">HH", in_entries, out_entries)
    elem += put(np.tile(tin, 3)) + put(clut) + put(np.tile(tout, 3))
    stages = [("curves", [tin] * 3), ("clut", clut), ("curves", [tout] * 3)]
    name = "%s-%s-v%d-g%d-i%d-o%d-s%d" % ("mft2" if wide else "mft1", pcs.decode().strip(), version, grid, in_entries, out_entries, seed)
    icc = E.icc_profile((), (), pcs=pcs, version=version, extra=[(b"A2B0", elem)])
    return LutProfile(name, icc, stages, pcs, version, "mft2" if wide else "mft1")


def _curve_bytes(spec):
    e = E.curve(spec)
    return e + b"\0" * (-len(e) % 4)


def mab_profile(seed, pcs=b"XYZ ", version=4, grid=(9, 7, 5), a_curves="para", clut_bytes=2, m_curves=None, matrix=False):
    """lutAToB.  XYZ with `matrix`: A (gamma) - CLUT (twist) - M - matrix (colourants) - B; without a grid (grid=None): M (gamma)
    - matrix - B.  Otherwise A - CLUT (-> PCS) - B.  Curves: "para" (sRGB-like type 3 or plain type 0), "curv" (256 entries)."""
    dev = Device(seed)
    g = dev.gamma

    def gamma_specs(kind):
        if kind == "para":                                                         # one plain power, two sRGB-shaped (type 3) of that gamma
            a, b = 1 / 1.055, 0.055 / 1.055
            d = 0.04045
            c = (a * d + b) ** g / d
            return [("para", 0, [g]), ("para", 3, [g, a, b, c, d]), ("para", 3, [g, a, b, c, d])]
        return [("curv", [int(v) for v in _power_table(256, g)])] * 3
    identity = [("curv", [])] * 3
    stages, parts, offs = [], b"", {}
    head = 32

    def add(key, blob):
        nonlocal parts
        offs[key] = head + len(parts)
        parts += blob + b"\0" * (-len(blob) % 4)
    if grid is not None:
        specs = gamma_specs(a_curves)
        add("a", b"".join(_curve_bytes(s) for s in specs))
        stages.append(("curves", specs))
        lin = np.stack([E.curve_f64(specs[k], _grid_points(grid)[..., k]) for k in range(3)], axis=-1)
        if matrix:
            clut = np.round(dev.twisted(lin) * 65535).astype(np.uint16)
        else:
            clut = encode_pcs(dev.xyz(lin), pcs, "v4")
        if clut_bytes == 1:
            clut = (clut >> 8) * 257
        body = bytes(grid) + b"\0" * 13 + bytes([clut_bytes, 0, 0, 0])
        body += b"".join(struct.pack(">H", int(v)) for v in clut.ravel()) if clut_bytes == 2 else bytes(int(v) >> 8 for v in clut.ravel())
        add("c", body)
        stages.append(("clut", clut))
    if matrix:
        specs = gamma_specs(m_curves) if grid is None else ([("para", 0, [1.0])] * 3 if m_curves == "para" else [("curv", [0, 65535])] * 3)
        add("m", b"".join(_curve_bytes(s) for s in specs))
        stages.append(("curves", specs))
        m = dev.m / MAX_XYZ
        add("mat", b"".join(E.s15(v) for v in m.ravel()) + b"".join(E.s15(0) for _ in range(3)))
        stages.append(("matrix", np.round(m * 65536) / 65536, np.zeros(3)))
    add("b", b"".join(_curve_bytes(s) for s in identity))
    stages.append(("curves", identity))
    elem = b"mAB " + b"\0" * 4 + bytes([3, 3, 0, 0]) + struct.pack(">5I", offs["b"], offs.get("mat", 0), offs.get("m", 0), offs.get("c", 0), offs.get("a", 0)) + parts
    name = "mAB-%s-v%d-%s-%s%s%s-s%d" % (pcs.decode().strip(), version, "x".join(map(str, grid)) if grid else "nogrid", a_curves, clut_bytes,
                                        "-matrix-" + str(m_curves) if matrix else "", seed)
    icc = E.icc_profile((), (), pcs=pcs, version=version, extra=[(b"A2B0", elem)])
    return LutProfile(name, icc, stages, pcs, version, "mAB")


def gray_profile(trc, version=2, pcs=b"XYZ ", extra=()):
    """A GRAY profile with `trc` (an E.curve spec) under kTRC."""
    return E.icc_profile((), (), space=b"GRAY", pcs=pcs, version=version, extra=[(b"kTRC", E.curve(trc))] + list(extra))


GRAY_TRCS = {
    "identity": ("curv", []),
    "gamma2.2": ("gamma", 2.2),
    "gamma1.8": ("gamma", 1.8),
    "table": ("curv", [int(round(65535 * (i / 255) ** 2.2)) for i in range(256)]),
    "dotgain": ("curv", [int(round(65535 * ((i / 63) ** 1.75 * 0.9 + (i / 63) * 0.1))) for i in range(64)]),
    "para0": ("para", 0, [2.2]),
    "para1": ("para", 1, [2.2, 1.0, 0.0]),
    "para2": ("para", 2, [2.2, 1.0, 0.0, 0.0]),
    "para3": ("para", 3, [2.4, 1 / 1.055, 0.055 / 1.055, 1 / 12.92, 0.04045]),
    "para4": ("para", 4, [2.4, 1 / 1.055, 0.055 / 1.055, 1 / 12.92, 0.04045, 0.0, 0.0]),
}


def families():
    """name -> the profiles of one family (an element type and a connection space), every variant the tests cover"""
    f = {}
    f["mft1-XYZ"] = [mft_profile(1, wide=False, grid=9), mft_profile(2, wide=False, grid=17, version=4)]
    f["mft1-Lab"] = [mft_profile(3, wide=False, pcs=b"Lab ", grid=17), mft_profile(4, wide=False, pcs=b"Lab ", grid=9, version=4)]
    f["mft2-XYZ"] = [mft_profile(5, grid=17, in_entries=256, out_entries=256), mft_profile(6, grid=9, in_entries=4096, out_entries=2, version=4),
                     mft_profile(7, grid=3, in_entries=2, out_entries=4096), mft_profile(8, grid=2, in_entries=256, out_entries=256)]
    f["mft2-Lab"] = [mft_profile(9, pcs=b"Lab ", grid=17, in_entries=256, out_entries=2), mft_profile(10, pcs=b"Lab ", grid=9, in_entries=4096, out_entries=256, version=4),
                     mft_profile(11, pcs=b"Lab ", grid=17, in_entries=2, out_entries=2)]
    f["mAB-XYZ"] = [mab_profile(12, grid=(9, 7, 5), a_curves="para", matrix=True, m_curves="para"), mab_profile(13, grid=(17, 17, 17), a_curves="curv", clut_bytes=1, matrix=True, m_curves="curv"),
                    mab_profile(14, grid=None, matrix=True, m_curves="para"), mab_profile(15, grid=(9, 9, 9), a_curves="curv", version=2),
                    mab_profile(16, grid=(5, 9, 17), a_curves="para")]
    f["mAB-Lab"] = [mab_profile(17, pcs=b"Lab ", grid=(17, 9, 9), a_curves="para"), mab_profile(18, pcs=b"Lab ", grid=(9, 17, 17), a_curves="curv", clut_bytes=1)]
    return f
