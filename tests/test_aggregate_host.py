"""The aggregate entry points' host side (no GPU): what each call accepts and
what it refuses with PNR_EINVAL before any launch.  Argument structs are filled
with a fake 16-B aligned non-null pointer; nothing is dereferenced, and every
accepted call has n_max = 0 (or no P1 rows), which returns before any HIP call.

The messages are matched by the part after their `aggregate...:` prefix."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pointnerf_amd", "libpnr.so")

FAKE = 0x1000        # non-null, 16-B aligned, never dereferenced
ODD = FAKE + 4       # non-null, not 16-B aligned
N_POINTS = 100

MLP_PTRS = ("w1af", "w1bf", "w2f", "b2", "w3f", "b3", "w4f", "b4", "wa", "ba", "wc1f", "bc1", "wc2f", "bc2", "wc3f",
            "bc3")
SAVED_REQUIRED = ("h1", "h2", "h3", "h4", "pe5", "x3e", "pa", "wt", "wn", "prow", "hid", "vpe", "hc1", "hc2", "hc3",
                  "vmask", "mask")
SAVED_ALIGNED = ("h1", "h2", "h3", "h4", "hid", "hc1", "hc2", "hc3")
X3_PACKS = ("w1bx", "w2x", "w3x", "w4x")
H2_PACKS = ("w1bh", "w2h", "w3h", "w4h")
COLOUR_PACKS = ("wc1a", "wc1b", "wc2h", "wc3h")

FWD = ("pnr_aggregate_fwd", "pnr_aggregate_fwd_x3", "pnr_aggregate_fwd_h2", "pnr_aggregate_fwd_masked",
       "pnr_aggregate_fwd_train", "pnr_aggregate_fwd_train_x3", "pnr_aggregate_fwd_train_h2",
       "pnr_aggregate_fwd_train_h2_guarded", "pnr_aggregate_fwd_train_masked")
X3 = tuple(n for n in FWD if n.endswith("_x3"))
H2 = tuple(n for n in FWD if "_h2" in n)
MASKED = tuple(n for n in FWD if n.endswith("_masked"))
TRAIN = tuple(n for n in FWD if "_train" in n)
BWD_PAIRS = ("pnr_aggregate_bwd_pairs", "pnr_aggregate_bwd_pairs_x3", "pnr_aggregate_bwd_pairs_h2")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", ROOT, "-j8", "pointnerf_amd/libpnr.so"])
    from pointnerf_amd import _lib
    _lib.lib()
    return _lib


def _ref(x):
    return None if x is None else ctypes.byref(x)


class Call:
    """The arguments of one aggregate entry point, valid and with n_max = 0 until a case changes them."""

    def __init__(self, L, name):
        self.L, self.name = L, name
        self.pts = L.Points()
        self.pts.n = N_POINTS
        for f in ("xyz", "pers", "emb"):      # pers given, no camera: dropping pers leaves neither
            setattr(self.pts, f, FAKE)
        self.s = L.Samples()
        for f in ("sample_w", "sample_p", "dirs"):
            setattr(self.s, f, FAKE)
        self.s.pidx = None if name in MASKED else FAKE
        self.s.n_max, self.s.dir_div, self.s.K = 0, 1, 8
        self.w = L.Mlp()
        for f in MLP_PTRS:
            setattr(self.w, f, FAKE)
        self.w.neg_slope = 0.01
        self.wx = L.MlpX3()
        for f in X3_PACKS:
            setattr(self.wx, f, FAKE)
        self.wh = L.MlpH2()
        for f in H2_PACKS:
            setattr(self.wh, f, FAKE)
        self.wh.scale[:] = [1.0, 0.5, 2.0, 1.0]
        self.wh.range_flag = FAKE
        self.pair_mask = FAKE
        self.saved = L.AggSaved()
        for f in SAVED_REQUIRED:
            setattr(self.saved, f, FAKE)
        self.wb = L.MlpBwd()
        for f in ("w4t", "w3t", "w2t", "w3e"):
            setattr(self.wb, f, FAKE)
        self.wbx = L.MlpBwdX3()
        for f in ("w4tx", "w3tx", "w2tx"):
            setattr(self.wbx, f, FAKE)
        self.wbh = L.MlpBwdH2()
        for f in ("w4th", "w3th", "w2th", "scale"):
            setattr(self.wbh, f, FAKE)
        self.out_feat = self.scratch = FAKE
        nb = ctypes.c_size_t(0)
        assert L.lib().pnr_aggregate_scratch_bytes(0, N_POINTS, ctypes.byref(nb)) == L.PNR_OK and nb.value > 0
        self.scratch_bytes = nb.value
        # backward buffers: d_feat, d_hid, dz1..dz4, dpa, d_p1, d_color, d_dir, d_conf
        self.bufs = dict(d_feat=FAKE, d_hid=FAKE, dz1=FAKE, dz2=FAKE, dz3=FAKE, dz4=FAKE, dpa=FAKE, d_p1=FAKE,
                         d_color=FAKE, d_dir=FAKE, d_conf=FAKE)
        self.d_pe = self.d_xyz = self.w3e = self.g_pair = FAKE

    def args(self):
        n = self.name
        head = [_ref(self.pts), _ref(self.s), _ref(self.w)]
        if n in FWD:
            mid = []
            if n in X3:
                mid.append(_ref(self.wx))
            if n in H2:
                mid.append(_ref(self.wh))
            if n in MASKED:
                mid.append(self.pair_mask)
            if n in TRAIN:
                mid.append(_ref(self.saved))
            return head + mid + [self.out_feat, FAKE, FAKE, self.scratch, self.scratch_bytes, None]
        if n == "pnr_point_pre_h2":
            return [_ref(self.pts), _ref(self.wh), self.scratch, self.scratch_bytes, None]
        if n in BWD_PAIRS:
            mid = [_ref(self.wb)]
            if n.endswith("_x3"):
                mid.append(_ref(self.wbx))
            if n.endswith("_h2"):
                mid.append(_ref(self.wbh))
            return head + mid + [_ref(self.saved)] + list(self.bufs.values()) + [None]
        if n == "pnr_aggregate_bwd_xyz":
            return head + [_ref(self.saved), self.bufs["d_feat"], self.bufs["d_hid"], self.d_pe, self.d_xyz, None]
        assert n == "pnr_aggregate_bwd_extras_rows"
        return head + [_ref(self.saved), self.w3e, self.bufs["dz3"], self.g_pair, None]

    def run(self):
        return getattr(self.L.lib(), self.name)(*self.args())


def _set(obj, field, value):
    def f(c):
        setattr(getattr(c, obj), field, value)
    return f


def _drop(obj):
    def f(c):
        setattr(c, obj, None)
    return f


def _scale(i, v):
    def f(c):
        c.wh.scale[i] = v
    return f


def _cscale(i, v):
    def f(c):
        c.wh.cscale[i] = v
    return f


def _colour(ptrs=COLOUR_PACKS, cscale=(1.0, 1.0, 1.0)):
    def f(c):
        for n in ptrs:
            setattr(c.wh, n, FAKE)
        c.wh.cscale[:] = list(cscale)
    return f


def _both(*fs):
    def f(c):
        for g in fs:
            g(c)
    return f


def _short_scratch(c):
    c.scratch_bytes -= 1


def _used_without_map(c):
    c.pts.used, c.pts.n_used, c.pts.used_map = FAKE, 10, None


def _buf(name, v):
    def f(c):
        c.bufs[name] = v
    return f


# (case id, entry points, change, fragment of pnr_last_error())
COMMON = [
    ("null-pts", FWD, _drop("pts"), b"null pointer"),
    ("null-samples", FWD, _drop("s"), b"null pointer"),
    ("null-mlp", FWD, _drop("w"), b"null pointer"),
    ("null-out-feat", FWD, _drop("out_feat"), b"null pointer"),
    ("no-xyz", FWD, _set("pts", "xyz", None), b"xyz/emb required"),
    ("no-emb", FWD, _set("pts", "emb", None), b"xyz/emb required"),
    ("no-sample-w", FWD, _set("s", "sample_w", None), b"sample arrays required"),
    ("no-sample-p", FWD, _set("s", "sample_p", None), b"sample arrays required"),
    ("no-dirs", FWD, _set("s", "dirs", None), b"sample arrays required"),
    ("K-0", FWD, _set("s", "K", 0), b"K=0 unsupported"),
    ("K-9", FWD, _set("s", "K", 9), b"K=9 unsupported"),
    ("dir-div-0", FWD, _set("s", "dir_div", 0), b"dir_div must be >= 1"),
    ("emb-misaligned", FWD, _set("pts", "emb", ODD), b"emb must be 16-B aligned"),
    ("scratch-null", FWD, _drop("scratch"), b"aligned scratch required"),
    ("scratch-misaligned", FWD, lambda c: setattr(c, "scratch", ODD), b"aligned scratch required"),
    ("no-points", FWD, _set("pts", "n", 0), b"empty point table"),
    ("used-without-map", FWD, _used_without_map, b"used list needs used_map"),
    ("scratch-one-byte-short", FWD, _short_scratch, b"scratch too small"),
    ("no-pers-no-camera", tuple(n for n in FWD if n not in MASKED), _set("pts", "pers", None),
     b"need pers or camera"),
    ("masked-no-pers", MASKED, _set("pts", "pers", None), b"pers required"),
    ("masked-null-mask", MASKED, _drop("pair_mask"), b"null pair_mask"),
    ("masked-with-pidx", MASKED, _set("s", "pidx", FAKE), b"pidx must be NULL"),
    ("split-no-pidx", X3 + H2, _set("s", "pidx", None), b"pidx required"),
    ("x3-null-struct", X3, _drop("wx"), b"null split weight pack"),
    ("h2-null-struct", ("pnr_aggregate_fwd_h2", "pnr_aggregate_fwd_train_h2"), _drop("wh"),
     b"null split weight pack"),
    ("slope-negative", X3 + H2, _set("w", "neg_slope", -0.01), b"LeakyReLU slope must be in [0, 1]"),
    ("slope-above-1", X3 + H2, _set("w", "neg_slope", 1.5), b"LeakyReLU slope must be in [0, 1]"),
    ("h2-scale-zero", H2, _scale(2, 0.0), b"bad layer scale 2"),
    ("h2-scale-1e30", H2, _scale(1, 1e30), b"bad layer scale 1"),
    ("saved-null-struct", TRAIN, _drop("saved"), b"null saved struct"),
    ("guarded-null-struct", ("pnr_aggregate_fwd_train_h2_guarded",), _drop("wh"), b"range_flag required"),
    ("guarded-no-flag", ("pnr_aggregate_fwd_train_h2_guarded",), _set("wh", "range_flag", None),
     b"range_flag required"),
    # the inference h2 call checks the optional packs in front of its n_max = 0 return
    ("h2-w1ah-misaligned", ("pnr_aggregate_fwd_h2",), _both(_set("wh", "w1ah", ODD), _set("wh", "scale1a", 1.0)),
     b"bad block1.0 point-half pack"),
    ("h2-w1ah-scale-zero", ("pnr_aggregate_fwd_h2",), _both(_set("wh", "w1ah", FAKE), _set("wh", "scale1a", 0.0)),
     b"bad block1.0 point-half pack"),
    ("h2-w1ah-scale-1e30", ("pnr_aggregate_fwd_h2",), _both(_set("wh", "w1ah", FAKE), _set("wh", "scale1a", 1e30)),
     b"bad block1.0 point-half pack"),
    ("h2-colour-misaligned", ("pnr_aggregate_fwd_h2",), _both(_colour(), _set("wh", "wc2h", ODD)),
     b"colour packs must be 16-B aligned"),
    ("h2-colour-scale-zero", ("pnr_aggregate_fwd_h2",), _colour(cscale=(1.0, 0.0, 1.0)), b"colour layer scale 1"),
    ("h2-colour-scale-1e30", ("pnr_aggregate_fwd_h2",), _colour(cscale=(1.0, 1.0, 1e30)), b"colour layer scale 2"),
]
COMMON += [("null-weight-" + f, FWD, _set("w", f, None), b"null weight") for f in MLP_PTRS]
COMMON += [("x3-null-" + f, X3, _set("wx", f, None), b"null split weight pack") for f in X3_PACKS]
COMMON += [("x3-misaligned-" + f, X3, _set("wx", f, ODD), b"split packs must be 16-B aligned") for f in X3_PACKS]
COMMON += [("h2-null-" + f, H2, _set("wh", f, None), b"null split weight pack") for f in H2_PACKS]
COMMON += [("h2-misaligned-" + f, H2, _set("wh", f, ODD), b"split packs must be 16-B aligned") for f in H2_PACKS]
COMMON += [("saved-null-" + f, TRAIN, _set("saved", f, None), b"null saved array") for f in SAVED_REQUIRED]
COMMON += [("saved-misaligned-" + f, TRAIN, _set("saved", f, ODD), b"saved activations must be 16-B aligned")
           for f in SAVED_ALIGNED]

BWD_PAIRS_ONLY, BWD_X3_ONLY, BWD_H2_ONLY = BWD_PAIRS[:1], BWD_PAIRS[1:2], BWD_PAIRS[2:]
BWD = [
    ("null-pts", BWD_PAIRS, _drop("pts"), b"null pointer"),
    ("null-samples", BWD_PAIRS, _drop("s"), b"null pointer"),
    ("null-mlp", BWD_PAIRS, _drop("w"), b"null pointer"),
    ("null-wb", BWD_PAIRS, _drop("wb"), b"null pointer"),
    ("saved-null-struct", BWD_PAIRS, _drop("saved"), b"null saved struct"),
    ("null-wa", BWD_PAIRS, _set("w", "wa", None), b"null weight"),
    ("fp32-null-w3e", BWD_PAIRS_ONLY, _set("wb", "w3e", None), b"null weight"),
    ("fp32-null-w4t", BWD_PAIRS_ONLY, _set("wb", "w4t", None), b"null weight"),
    ("fp32-null-w3t", BWD_PAIRS_ONLY, _set("wb", "w3t", None), b"null weight"),
    ("fp32-null-w2t", BWD_PAIRS_ONLY, _set("wb", "w2t", None), b"null weight"),
    ("x3-null-struct", BWD_X3_ONLY, _drop("wbx"), b"null split weight packs"),
    ("h2-null-struct", BWD_H2_ONLY, _drop("wbh"), b"null split weight packs"),
    ("h2-null-scale", BWD_H2_ONLY, _set("wbh", "scale", None), b"null or unaligned split weight pack"),
    ("null-d-feat", BWD_PAIRS, _buf("d_feat", None), b"null buffer"),
    ("null-d-hid", BWD_PAIRS, _buf("d_hid", None), b"null buffer"),
    ("null-dpa", BWD_PAIRS, _buf("dpa", None), b"null buffer"),
    ("d-hid-misaligned", BWD_PAIRS, _buf("d_hid", ODD), b"gradient buffers must be 16-B aligned"),
    ("no-dirs", BWD_PAIRS, _set("s", "dirs", None), b"sample dirs required"),
    ("dir-div-0", BWD_PAIRS, _set("s", "dir_div", 0), b"sample dirs required"),
    ("K-0", BWD_PAIRS, _set("s", "K", 0), b"K=0 unsupported"),
    ("K-9", BWD_PAIRS, _set("s", "K", 9), b"K=9 unsupported"),
]
BWD += [("x3-null-" + f, BWD_X3_ONLY, _set("wbx", f, None), b"null or unaligned split weight pack")
        for f in ("w4tx", "w3tx", "w2tx")]
BWD += [("x3-misaligned-" + f, BWD_X3_ONLY, _set("wbx", f, ODD), b"null or unaligned split weight pack")
        for f in ("w4tx", "w3tx", "w2tx")]
BWD += [("h2-null-" + f, BWD_H2_ONLY, _set("wbh", f, None), b"null or unaligned split weight pack")
        for f in ("w4th", "w3th", "w2th")]
BWD += [("h2-misaligned-" + f, BWD_H2_ONLY, _set("wbh", f, ODD), b"null or unaligned split weight pack")
        for f in ("w4th", "w3th", "w2th")]
BWD += [("null-" + f, BWD_PAIRS, _buf(f, None), b"null buffer") for f in ("dz1", "dz2", "dz3", "dz4")]
BWD += [(f + "-misaligned", BWD_PAIRS, _buf(f, ODD), b"gradient buffers must be 16-B aligned")
        for f in ("dz1", "dz2", "dz3", "dz4")]
BWD += [("saved-null-" + f, BWD_PAIRS, _set("saved", f, None), b"null saved array") for f in SAVED_REQUIRED]
BWD += [("saved-misaligned-" + f, BWD_PAIRS, _set("saved", f, ODD), b"saved activations must be 16-B aligned")
        for f in SAVED_ALIGNED]

XYZ = ("pnr_aggregate_bwd_xyz",)
ROWS = ("pnr_aggregate_bwd_extras_rows",)
PRE = ("pnr_point_pre_h2",)


def _pre_no_rows(c):
    c.pts.n = 0


def _pre(f):
    """pnr_point_pre_h2 cases start from a valid pack."""
    return _both(_set("wh", "w1ah", FAKE), _set("wh", "scale1a", 1.0), f)


def _pre_scratch(nbytes):
    def f(c):
        c.scratch_bytes = nbytes
    return f


OTHER = [
    ("null-pts", XYZ, _drop("pts"), b"null argument"),
    ("null-samples", XYZ, _drop("s"), b"null argument"),
    ("null-mlp", XYZ, _drop("w"), b"null argument"),
    ("null-saved", XYZ, _drop("saved"), b"null argument"),
    ("null-d-feat", XYZ, _buf("d_feat", None), b"null argument"),
    ("null-d-hid", XYZ, _buf("d_hid", None), b"null argument"),
    ("null-d-pe", XYZ, _drop("d_pe"), b"null argument"),
    ("null-d-xyz", XYZ, _drop("d_xyz"), b"null argument"),
    ("no-xyz", XYZ, _both(_set("pts", "campos", FAKE), _set("pts", "camrot", FAKE), _set("pts", "xyz", None)),
     b"need xyz and the camera tables"),
    ("no-campos", XYZ, _set("pts", "camrot", FAKE), b"need xyz and the camera tables"),
    ("no-camrot", XYZ, _set("pts", "campos", FAKE), b"need xyz and the camera tables"),
    ("K-9", XYZ, _both(_set("pts", "campos", FAKE), _set("pts", "camrot", FAKE), _set("s", "K", 9)), b"K > 8"),
    ("null-pts", ROWS, _drop("pts"), b"null pointer"),
    ("null-samples", ROWS, _drop("s"), b"null pointer"),
    ("null-mlp", ROWS, _drop("w"), b"null pointer"),
    ("null-saved", ROWS, _drop("saved"), b"null pointer"),
    ("null-prow", ROWS, _set("saved", "prow", None), b"null pointer"),
    ("null-w3e", ROWS, _drop("w3e"), b"null pointer"),
    ("null-dz3", ROWS, _both(_set("s", "n_max", 64), _buf("dz3", None)), b"dz3 / g_pair must be 16-B aligned"),
    ("null-g-pair", ROWS, _both(_set("s", "n_max", 64), _drop("g_pair")), b"dz3 / g_pair must be 16-B aligned"),
    ("dz3-misaligned", ROWS, _both(_set("s", "n_max", 64), _buf("dz3", ODD)), b"dz3 / g_pair must be 16-B aligned"),
    ("g-pair-misaligned", ROWS, _both(_set("s", "n_max", 64), lambda c: setattr(c, "g_pair", ODD)),
     b"dz3 / g_pair must be 16-B aligned"),
    ("no-dirs", ROWS, _set("s", "dirs", None), b"sample dirs required"),
    ("dir-div-0", ROWS, _set("s", "dir_div", 0), b"sample dirs required"),
    ("null-pts", PRE, _pre(_drop("pts")), b"null pointer"),
    ("null-wh", PRE, _drop("wh"), b"null pointer"),
    ("no-emb", PRE, _pre(_set("pts", "emb", None)), b"null pointer"),
    ("null-scratch", PRE, _pre(_drop("scratch")), b"null pointer"),
    ("null-w1ah", PRE, _set("wh", "scale1a", 1.0), b"bad block1.0 point-half pack"),
    ("w1ah-misaligned", PRE, _pre(_set("wh", "w1ah", ODD)), b"bad block1.0 point-half pack"),
    ("w1ah-scale-zero", PRE, _pre(_set("wh", "scale1a", 0.0)), b"bad block1.0 point-half pack"),
    ("w1ah-scale-1e30", PRE, _pre(_set("wh", "scale1a", 1e30)), b"bad block1.0 point-half pack"),
    ("emb-misaligned", PRE, _pre(_set("pts", "emb", ODD)), b"emb and scratch must be 16-B aligned"),
    ("scratch-misaligned", PRE, _pre(lambda c: setattr(c, "scratch", ODD)), b"emb and scratch must be 16-B aligned"),
    ("scratch-one-byte-short", PRE, _pre(_pre_scratch(N_POINTS * 256 * 4 - 1)), b"scratch too small"),
    ("negative-n-used", PRE, _pre(_both(_set("pts", "used", FAKE), _set("pts", "n_used", -1))),
     b"scratch too small"),
]


def _expand(table):
    return [pytest.param(name, change, frag, id=f"{name[4:]}-{cid}") for cid, names, change, frag in table
            for name in names]


@pytest.mark.parametrize("name", FWD + BWD_PAIRS + XYZ + ROWS)
def test_accepted_call_without_samples_returns_ok(L, name):
    c = Call(L, name)
    if name in XYZ:
        c.pts.campos = c.pts.camrot = FAKE
    assert c.run() == L.PNR_OK


def test_point_pre_h2_without_rows_returns_ok(L):
    c = Call(L, "pnr_point_pre_h2")
    _pre(_pre_no_rows)(c)
    assert c.run() == L.PNR_OK
    c = Call(L, "pnr_point_pre_h2")     # an empty used list
    _pre(_both(_set("pts", "used", FAKE), _set("pts", "n_used", 0)))(c)
    assert c.run() == L.PNR_OK


@pytest.mark.parametrize("name", FWD)
def test_camera_instead_of_pers_is_accepted(L, name):
    c = Call(L, name)
    c.pts.pers, c.pts.campos, c.pts.camrot = None, FAKE, FAKE
    if name in MASKED:      # the mirror path has no camera
        assert c.run() == L.PNR_EINVAL and b"pers required" in L.lib().pnr_last_error()
    else:
        assert c.run() == L.PNR_OK


@pytest.mark.parametrize("name,change,frag", _expand(COMMON + BWD + OTHER))
def test_refusal_before_any_launch(L, name, change, frag):
    c = Call(L, name)
    change(c)
    assert c.run() == L.PNR_EINVAL
    assert frag in L.lib().pnr_last_error(), L.lib().pnr_last_error()


def test_used_list_with_map_is_accepted(L):
    for name in FWD:
        c = Call(L, name)
        c.pts.used, c.pts.n_used, c.pts.used_map = FAKE, 10, FAKE
        assert c.run() == L.PNR_OK, name
        c.pts.n_used = N_POINTS + 1
        assert c.run() == L.PNR_EINVAL and b"used list needs used_map" in L.lib().pnr_last_error(), name


def test_full_optional_h2_packs_are_accepted(L):
    for name in H2:
        c = Call(L, name)
        _both(_colour(), _set("wh", "w1ah", FAKE), _set("wh", "scale1a", 0.25))(c)
        assert c.run() == L.PNR_OK, name


@pytest.mark.parametrize("missing", COLOUR_PACKS[1:])
def test_inference_h2_refuses_partial_colour_packs(L, missing):
    """pnr_aggregate_fwd_h2: wc1a set with another colour pack missing is an error, at n_max = 0 too."""
    c = Call(L, "pnr_aggregate_fwd_h2")
    _both(_colour(), _set("wh", missing, None))(c)
    assert c.run() == L.PNR_EINVAL
    assert b"partial colour-branch packs" in L.lib().pnr_last_error()


def test_inference_h2_without_wc1a_takes_the_fp32_colour_branch(L):
    c = Call(L, "pnr_aggregate_fwd_h2")
    _both(_colour(), _set("wh", "wc1a", None))(c)
    assert c.run() == L.PNR_OK


@pytest.mark.parametrize("name", ("pnr_aggregate_fwd_train_h2", "pnr_aggregate_fwd_train_h2_guarded"))
@pytest.mark.parametrize("missing", COLOUR_PACKS)
def test_training_h2_accepts_partial_colour_packs(L, name, missing):
    """pnr_aggregate_fwd_train_h2(_guarded): a partial colour-pack set selects the fp32 colour
    branch, it is no error -- the asymmetry to the inference call, stated as such."""
    c = Call(L, name)
    _both(_colour(), _set("wh", missing, None))(c)
    assert c.run() == L.PNR_OK


@pytest.mark.parametrize("name", ("pnr_aggregate_fwd_train_h2", "pnr_aggregate_fwd_train_h2_guarded"))
def test_training_h2_checks_optional_packs_only_with_samples(L, name):
    """The training call's w1ah / saved x1 / colour-pack checks sit behind its n_max = 0 return."""
    c = Call(L, name)
    _both(_colour(cscale=(0.0, 0.0, 0.0)), _set("wh", "wc2h", ODD), _set("wh", "w1ah", ODD),
          _set("saved", "x1", ODD))(c)
    assert c.run() == L.PNR_OK
