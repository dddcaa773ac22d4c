"""Case tables, input generators and the float64 statement of one segment for the seam tests of dd3d_conv2d_igemm_f32
(tests/test_conv_seam_gpu.py on the GPU; tests/test_conv_seam_cases.py proves on the CPU that the tables exercise what they claim).

What the seam tests are about: a single-segment ConvOp launch carries its descriptor in the kernel arguments (`ka.single`: m0 = mt * BM,
no memory read), so every older single-segment test leaves the path the model runs -- s = segs[tiles[2 mt]], m0 = tiles[2 mt + 1] --
untouched.  The launches below have several unequal segments, forced tiles, split-K, residual / output forms mixed inside a launch, and
the epilogue options of the predictors (lower clamp `lo`, `n_limit`, `in_relu`, the half-range guard).

A launch is a dict (see `launch`), a segment a dict (see `seg`).  Every segment draws its data from a generator seeded by its own tag,
never by its position, so the same segment can be placed alone, first, in the middle or last (group B).

The reference of one segment, float64 on the CPU:
    y = conv2d(relu?(x), w) * scale + bias (+ residual);  out = max(y, lo'),  lo' = max(lo, 0) if relu else lo
compared on the channels below n_limit only."""
import functools
import zlib

import torch
import torch.nn.functional as F

from dd3d_amd import hip
from tests.test_conv_planes_gpu import MODES  # the project's per-mode bars: {name: (math, rtol)}

SENT_F32 = -777.0   # f32 channels outside a segment's slice
SENT_PLANE = 0x1234  # plane chunk images outside a segment's slice
F32_RTOL = 2e-5     # bar of the f32-input kernels (test_conv_gpu.py)
# a planes-only output carries its own rounding on top of the convolution's (test_conv_planes_gpu.py::test_residual_forms)
OUT_STEP = {hip.MATH_F32: 0.0, hip.MATH_BF16X3: 0.0, hip.MATH_F16X2: 2.0**-21, hip.MATH_BF16X2: 2.0**-15, hip.MATH_BF16: 2.0**-8}

FAMILIES = ("f32", "x3f32", "pertap", "row")  # f32 MFMA; bf16x3 splitting f32 input on the fly; split planes per tap / row-shared
PLANE_FAMILIES = ("pertap", "row")
W8_TILES = (hip.TILE_256x256_W8, hip.TILE_192x256_W8)  # 8 waves x 8 accumulator blocks: one- and two-term modes, no residual, no split-K


def seg(tag, B, H, W, filt=0, res=None, out="both", n_limit=0, lo=None):
    """One segment.  (B, H, W): its INPUT map; `filt`: which of the launch's filters it uses; `res`: None | "f32" | "planes" |
    "planes_up"; `out`: "f32" | "planes" | "both" (the f32-input families write f32 whatever this says); `lo`: None or "mixed"."""
    return dict(tag=tag, B=B, H=H, W=W, filt=filt, res=res, out=out, n_limit=n_limit, lo=lo)


def launch(name, family, mode, tile, splitk, segs, Cin=64, N=96, k=3, stride=1, pad=1, relu=True, in_relu=False, data="randn", raise_bias=None):
    """One ConvOp.  `mode`: a key of MODES for the split-plane families, None for the two f32-input ones.  `tile` / `splitk`: forced, or
    None for the model's own choice.  `data`: the input generator (`_seg_data`).  `raise_bias`: (segment, channel, value)."""
    assert family in FAMILIES and (mode in MODES) == (family in PLANE_FAMILIES), (name, family, mode)
    return dict(name=name, family=family, mode=mode, tile=tile, splitk=splitk, segs=list(segs), Cin=Cin, N=N, k=k, stride=stride, pad=pad,
                relu=relu, in_relu=in_relu, data=data, raise_bias=raise_bias)


def case_id(L):
    t = "auto" if L["tile"] is None else hip.TILE_NAMES[L["tile"]]
    return f"{L['name']}-{L['family']}-{L['mode'] or 'f32in'}-{t}-sk{L['splitk'] or 'auto'}"


def math_of(L):
    return {"f32": hip.MATH_F32, "x3f32": hip.MATH_BF16X3}[L["family"]] if L["mode"] is None else MODES[L["mode"]][0]


def rtol_of(L):
    return MODES[L["mode"]][1] if L["family"] in PLANE_FAMILIES else F32_RTOL


def out_hw(L, s):
    return (s["H"] + 2 * L["pad"] - L["k"]) // L["stride"] + 1, (s["W"] + 2 * L["pad"] - L["k"]) // L["stride"] + 1


def seg_m(L, s):
    ho, wo = out_hw(L, s)
    return s["B"] * ho * wo


def row_kernel_runs(L):
    """Whether the library takes the row-shared kernel for this launch (csrc/conv_planes_row.hip::conv_planes_row_applicable)."""
    nk = L["k"] * L["k"] * L["Cin"] // 32
    sk = L["splitk"] or 1
    return L["family"] == "row" and (L["k"], L["stride"], L["pad"]) == (3, 1, 1) and (sk == 1 or -(-nk // sk) % 3 == 0)


# ------------------------------------------------------------------------------------------------ data
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32("/".join(str(k) for k in key).encode()))


LO_CYCLE = (float("-inf"), 0.0, 0.25, -0.25)  # "mixed": no clamp, zero, a positive and a negative finite bound, channel after channel


@functools.lru_cache(maxsize=None)
def _filter(data, filt, n_rows, N, Cin, k):
    """OIHW filter of N rows; rows >= n_rows are zero (a narrow predictor group padded to the launch's N)."""
    g = _gen("filter", data, filt, n_rows, Cin, k)
    K = Cin * k * k
    if data == "zero_w":
        return torch.zeros(N, Cin, k, k)
    if data == "bimodal":
        # a dominant centre tap along the direction a[c] (see _seg_data) + a small dense random part: conv = +-1 + noise of std ~0.06
        a = _bimodal_dir(Cin)
        w = torch.randn(N, Cin, k, k, generator=g) * (0.06 / (1.05 * K**0.5))
        d = (torch.randint(0, 2, (N, ), generator=g) * 2 - 1).float()
        w[:, :, k // 2, k // 2] += d[:, None] * a[None, :] / float((a * a).sum())
    else:
        w = torch.randn(N, Cin, k, k, generator=g) / K**0.5
    w[n_rows:] = 0
    return w


def _bimodal_dir(Cin):
    g = _gen("bimodal_dir", Cin)
    return (torch.rand(Cin, generator=g) + 0.5) * (torch.randint(0, 2, (Cin, ), generator=g) * 2 - 1).float()


@functools.lru_cache(maxsize=None)
def _seg_data(data, tag, B, H, W, Ho, Wo, Cin, N, n, res, lo):
    """Everything one segment reads, from a generator seeded by its tag.  `n`: channels it stores.
      randn    x ~ N(0, 1), scale in [0.5, 1.5), bias ~ N(0, 1): about half of a rectified output is clamped
      neg      x ~ N(-1, 1): five entries in six are negative (group E)
      bimodal  x = +-a[c] per pixel + 0.1 N(0, 1): with the matching filter every output is near +-scale, away from every `lo` (group D)
      zero_w   (zero filter) scale 1, bias 1.5: every stored value is 1.5 (group F)"""
    g = _gen("seg", data, tag, B, H, W, Cin, N)
    x = torch.randn(B, Cin, H, W, generator=g)
    scale, bias = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g)
    if data == "neg":
        x = x - 1.0
    elif data == "bimodal":
        sgn = (torch.randint(0, 2, (B, 1, H, W), generator=g) * 2 - 1).float()
        x = sgn * _bimodal_dir(Cin).view(1, Cin, 1, 1) + 0.1 * x
        scale, bias = 0.8 + 0.4 * (scale - 0.5), 0.1 * bias.clamp(-1, 1)
    elif data == "zero_w":
        scale, bias = torch.ones(N), torch.full((N, ), 1.5)
    r = None
    if res is not None:
        up = res == "planes_up"
        r = torch.randn(B, N, Ho // 2 if up else Ho, Wo // 2 if up else Wo, generator=g)
    lo_vec = None
    if lo == "mixed":
        lo_vec = torch.tensor([LO_CYCLE[(c + len(tag)) % 4] for c in range(N)])
    return dict(x=x, scale=scale, bias=bias, res=r, lo=lo_vec)


def seg_data(L, i):
    s = L["segs"][i]
    ho, wo = out_hw(L, s)
    d = dict(_seg_data(L["data"], s["tag"], s["B"], s["H"], s["W"], ho, wo, L["Cin"], L["N"], s["n_limit"] or L["N"], s["res"], s["lo"]))
    rb = L["raise_bias"]
    if rb is not None and rb[0] == i:
        d["bias"] = d["bias"].clone()
        d["bias"][rb[1]] = rb[2]
    d["w"] = _filter(L["data"], s["filt"], s["n_limit"] or L["N"], L["N"], L["Cin"], L["k"])
    return d


@functools.lru_cache(maxsize=None)
def _conv64(data, tag, filt, B, H, W, Ho, Wo, Cin, N, n, k, stride, pad, in_relu):
    x = _seg_data(data, tag, B, H, W, Ho, Wo, Cin, N, n, None, None)["x"].double()
    return F.conv2d(F.relu(x) if in_relu else x, _filter(data, filt, n, N, Cin, k)[:n].double(), None, stride=stride, padding=pad)


def reference(L, i, res=None):
    """float64 (out, lo', y) of segment i on its stored channels: out = max(y, lo') [B, n, Ho, Wo], lo' [n].  `res`: the residual VALUE the kernel adds
    ([B, >= n, Ho or Ho/2, Wo or Wo/2]; what the planes hold for a plane residual); default: the generated f32 residual."""
    s, d = L["segs"][i], seg_data(L, i)
    n = s["n_limit"] or L["N"]
    ho, wo = out_hw(L, s)
    acc = _conv64(L["data"], s["tag"], s["filt"], s["B"], s["H"], s["W"], ho, wo, L["Cin"], L["N"], n, L["k"], L["stride"], L["pad"], L["in_relu"])
    y = acc * d["scale"][:n].double().view(1, -1, 1, 1) + d["bias"][:n].double().view(1, -1, 1, 1)
    if s["res"] is not None:
        r = (d["res"] if res is None else res)[:, :n].double()
        if s["res"] == "planes_up":
            r = F.interpolate(r, scale_factor=2.0, mode="nearest")
        y = y + r
    lo = torch.full((n, ), float("-inf"), dtype=torch.float64) if d["lo"] is None else d["lo"][:n].double()
    if L["relu"]:
        lo = lo.clamp(min=0.0)
    return torch.maximum(y, lo.view(1, -1, 1, 1)), lo, y


def bar(L, ref, planes_only=False):
    """The absolute bar of one segment: the mode's relative bar (plus the output rounding of a planes-only output) times max(1, max |ref|)
    of THAT segment."""
    return (rtol_of(L) + (OUT_STEP[math_of(L)] if planes_only else 0.0)) * max(1.0, float(ref.abs().max()))


def decode_planes(p, f16, plane_scale):
    """int16 [chunks][M][NP][32] -> float32 [M][chunks * 32]: the value the planes hold (Buf.nchw's decode, largest term first)."""
    terms = p.view(torch.float16).float() / plane_scale if f16 else (p.to(torch.int32) << 16).view(torch.float32)
    x = terms[:, :, 0]
    for q in range(1, terms.shape[2]):
        x = x + terms[:, :, q]
    return x.permute(1, 0, 2).reshape(p.shape[1], -1)


# ------------------------------------------------------------------------------------------------ building a launch
def pad32(c):
    return (c + 31) // 32 * 32


class Built:
    pass


def build(L, device="cuda", dry_run=False):
    """Plan + ConvOp of launch L the way test_conv_planes_gpu.py / test_conv_gpu.py build theirs: inputs, residual sources and outputs are
    channel slices of wider buffers; outputs are pre-filled with sentinels.  On the device, the output storages of all segments are carved
    back to back out of ONE f32 and ONE int16 arena with a sentinel-filled guard frame after each, so a row written past the end of a
    segment (the tail of a partly filled last tile) lands in a guard or in a neighbour that is compared in full."""
    from dd3d_amd.engine import ConvOp, PlanBase, pack_filter
    fam, math = L["family"], math_of(L)
    planes = fam in PLANE_FAMILIES
    plan = PlanBase(device, dry_run=dry_run)
    plan.math = math if planes else hip.MATH_BF16X3  # (f32-only buffers: the f32-input kernels, as in test_conv_gpu.py)
    dev = plan.device
    R = Built()
    R.L, R.plan, R.ins, R.outs, R.ress, R.data = L, plan, [], [], [], []
    packed, segs, meta = {}, [], None
    for i, s in enumerate(L["segs"]):
        d = seg_data(L, i)
        R.data.append(d)
        n = s["n_limit"] or L["N"]
        if (s["filt"], n) not in packed:
            packed[(s["filt"], n)] = pack_filter(d["w"], dev)
        wp, meta = packed[(s["filt"], n)]
        ho, wo = out_hw(L, s)
        B, H, W, Cin = s["B"], s["H"], s["W"], L["Cin"]
        if planes:
            xin = plan.buf(f"x{i}", B, H, W, Cin + 64, kind="both")
            vin = xin.view(32, Cin)
        else:
            xin = plan.buf(f"x{i}", B, H, W, Cin + 8)
            vin = xin.view(4, Cin)
        xin.t[..., vin.c0:vin.c0 + Cin] = d["x"].permute(0, 2, 3, 1).to(dev)
        if planes:
            plan.split(vin, name=f"x{i}.split")
        form = s["out"] if planes and not s["n_limit"] else "f32"  # (ConvOp: n_limit segments write f32 maps only)
        if form == "f32":  # pitch > stored channels: [c0 + n, pitch) may belong to a neighbouring slice
            pitch = 4 + (n + 3) // 4 * 4 + 4
            yb = plan.buf(f"y{i}", B, ho, wo, pitch, kind="f32")
            vout = yb.view(4, pitch - 4)
        else:
            yb = plan.buf(f"y{i}", B, ho, wo, pad32(n) + 64, kind=form)
            vout = yb.view(32, pad32(n))
        sg = {"in": vin, "out": vout, "w": wp, "scale": d["scale"].to(dev), "bias": d["bias"].to(dev)}
        if d["lo"] is not None:
            sg["lo"] = d["lo"].to(dev)
        if s["n_limit"]:
            sg["n_limit"] = s["n_limit"]
        rb = None
        if s["res"] is not None:
            assert planes or s["res"] == "f32"
            r = d["res"]
            cp = pad32(L["N"])
            # the residual source is a 32-aligned slice of a wider buffer: res_pitch > the stored channel count
            rb = plan.buf(f"r{i}", r.shape[0], r.shape[2], r.shape[3], cp + 64, kind="f32" if s["res"] == "f32" else "both")
            rb.t.fill_(555.0)
            rb.t[..., 32:32 + cp] = 0.0
            rb.t[..., 32:32 + L["N"]] = r.permute(0, 2, 3, 1).to(dev)
            if s["res"] != "f32":
                plan.split(rb.view(32, cp), name=f"r{i}.split")
            sg["res"], sg["res_up"] = rb.view(32, cp), s["res"] == "planes_up"
        segs.append(sg)
        R.ins.append(xin)
        R.outs.append((yb, vout, n, form))
        R.ress.append(rb)
    if not dry_run:
        _carve_outputs(R)
    meta = dict(meta, N=L["N"], Npad=pad32(L["N"]))
    R.op = ConvOp(plan, meta, L["stride"], L["pad"], segs, L["relu"], tile=L["tile"], splitk=L["splitk"], name=L["name"], math=math, in_relu=L["in_relu"])
    plan.ops.append(R.op)
    return R


GUARD = 4096  # elements of the guard frame after every segment's storage (the frame after the last one takes a whole tile's tail)


def _carve_outputs(R):
    dev = R.plan.device
    for attr, dtype, sent in (("t", torch.float32, SENT_F32), ("p", torch.int16, SENT_PLANE)):
        bufs = [yb for yb, _, _, _ in R.outs if getattr(yb, attr) is not None]
        if not bufs:
            setattr(R, "arena_" + attr, None)
            continue
        tail = 256 * max(int(getattr(b, attr).numel() // (b.B * b.H * b.W)) for b in bufs)
        total = sum(int(getattr(b, attr).numel()) + GUARD for b in bufs) + tail
        arena = torch.full((total, ), sent, dtype=dtype, device=dev)
        guard = torch.ones(total, dtype=torch.bool)
        off = 0
        for b in bufs:
            old = getattr(b, attr)
            setattr(b, attr, arena[off:off + old.numel()].view(old.shape))
            guard[off:off + old.numel()] = False
            off += old.numel() + GUARD
        setattr(R, "arena_" + attr, (arena, guard))


# ------------------------------------------------------------------------------------------------ group A
def m_table(bm):
    """(tag, B, H, W) of the >= 5 segments of a 3 x 3 / stride 1 launch on a tile of `bm` rows: a 1 x 3 map, a partly filled last tile
    (M = bm - 1 where bm - 1 factorises inside 24 x 40, else the nearest below), an exactly full tile, a one-pixel last tile
    (M = bm + 1 where it factorises, else the next M with M % bm == 1), and three tiny images (a batch boundary inside a tile)."""
    return {
        64: [("m3", 1, 1, 3), ("m63", 1, 7, 9), ("m64", 1, 8, 8), ("m65", 1, 5, 13), ("b3", 3, 3, 5)],
        128: [("m3", 1, 1, 3), ("m126", 1, 9, 14), ("m128", 1, 8, 16), ("m385", 1, 11, 35), ("b3", 3, 3, 5)],  # 127, 129 = 3 x 43, 257: no map
        192: [("m3", 1, 1, 3), ("m190", 1, 10, 19), ("m192", 1, 12, 16), ("m385", 1, 11, 35), ("b3", 3, 3, 5)],  # 191, 193 are prime
        256: [("m3", 1, 1, 3), ("m255", 1, 15, 17), ("m256", 1, 16, 16), ("m513", 1, 19, 27), ("b3", 3, 3, 5)],  # 257 is prime
    }[bm]


S2_SHAPES = [("s2a", 1, 13, 21), ("s2b", 2, 5, 9), ("m3", 1, 1, 3), ("s2c", 1, 23, 39), ("b3", 3, 3, 5)]  # 3 x 3 / stride 2 on odd maps


def _a_segs(shapes, forms):
    # every segment its own input / scale / bias (its tag); the filters alternate between two (the predictors' per-level filters)
    return [seg(t, B, H, W, filt=i % 2, out=forms[i % len(forms)]) for i, (t, B, H, W) in enumerate(shapes)]


def _plane_tiles(mode, row):
    tiles = [hip.TILE_256x128, hip.TILE_64x64_W4, hip.TILE_256x128_T42, hip.TILE_128x256_T24]  # 8-wave, 4-wave, the two 8-block wave tiles
    if hip.MATH_PLANES[MODES[mode][0]] <= 2:
        tiles.append(hip.TILE_256x256_W8)
        if row:
            tiles.append(hip.TILE_192x256_W8)  # (instantiated for the row-shared kernel only)
    return tiles


def group_a():
    out = []
    forms = ("both", "planes", "f32")
    for fam, tiles in (("f32", (hip.TILE_128x128, hip.TILE_64x64, hip.TILE_64x128)),
                       ("x3f32", (hip.TILE_256x128, hip.TILE_128x128_W4, hip.TILE_64x64_W4, hip.TILE_128x64_K2))):
        for t in tiles:
            out.append(launch("a_s1", fam, None, t, 1, _a_segs(m_table(hip.TILE_SHAPES[t][0]), forms)))
    for fam in PLANE_FAMILIES:
        for mode in MODES:
            for t in _plane_tiles(mode, fam == "row"):
                out.append(launch("a_s1", fam, mode, t, 1, _a_segs(m_table(hip.TILE_SHAPES[t][0]), forms)))
    # split-K through the tile table.  Cin 96 = 27 K-tiles: splitk 3 keeps 9 per slice (the row kernel), splitk 2 gives 14 (the row
    # family falls back to the per-tap kernel).  The 8-wave 256-column tiles have no split-K form.
    for sk in (2, 3):
        out.append(launch("a_sk", "f32", None, hip.TILE_64x64, sk, _a_segs(m_table(64), forms), Cin=96))
        out.append(launch("a_sk", "x3f32", None, hip.TILE_128x128_W4, sk, _a_segs(m_table(128), forms), Cin=96))
        for fam in PLANE_FAMILIES:
            for mode in MODES:
                for t in (hip.TILE_128x64_W4, hip.TILE_256x128_T42):
                    out.append(launch("a_sk", fam, mode, t, sk, _a_segs(m_table(hip.TILE_SHAPES[t][0]), forms), Cin=96))
    # 1 x 1 and 3 x 3 / stride 2 on odd maps: one split-plane kernel serves both (the row-shared kernel is 3 x 3 / stride 1 only)
    for name, kw in (("a_1x1", dict(k=1, pad=0, Cin=128)), ("a_s2", dict(stride=2))):
        shapes = (lambda bm: m_table(bm)) if name == "a_1x1" else (lambda bm: S2_SHAPES)
        out.append(launch(name, "f32", None, hip.TILE_128x64, 1, _a_segs(shapes(128), forms), **kw))
        out.append(launch(name, "x3f32", None, hip.TILE_64x128, 1, _a_segs(shapes(64), forms), **kw))
        for mode in MODES:
            for t in (hip.TILE_256x128, hip.TILE_128x64_W4):
                out.append(launch(name, "pertap", mode, t, 1, _a_segs(shapes(hip.TILE_SHAPES[t][0]), forms), **kw))
    return out


# ------------------------------------------------------------------------------------------------ group B
B_TARGET = ("tgt", 2, 7, 9)  # 126 pixels: two 64-row tiles, the second partly filled, a batch boundary in the first
B_FILL = [("m3", 1, 1, 3), ("m65", 1, 5, 13), ("b3", 3, 3, 5)]
B_PLACES = {"alone": (), "first": (0, ), "middle": (2, ), "last": (3, )}


def group_b():
    """[(id, {place: launch})]: the target segment alone (descriptor by value) and first / in the middle / last among three others."""
    out = []
    cfgs = [("f32", None, hip.TILE_64x64), ("x3f32", None, hip.TILE_64x64_W4)] + [(f, m, hip.TILE_64x64_W4) for f in PLANE_FAMILIES for m in MODES]
    for fam, mode, tile in cfgs:
        for sk in (1, 3):  # Cin 96 = 27 K-tiles: 9 per slice
            places = {}
            for place, at in B_PLACES.items():
                shapes = list(B_FILL) if at else []
                shapes.insert(at[0] if at else 0, B_TARGET)
                places[place] = launch("b_" + place, fam, mode, tile, sk, [seg(t, B, H, W, out="both") for t, B, H, W in shapes], Cin=96)
            out.append((f"{fam}-{mode or 'f32in'}-sk{sk}", places))
    return out


# ------------------------------------------------------------------------------------------------ group C
def group_c():
    """Residual forms and output forms mixed inside one launch of the split-plane kernels."""
    out = []
    for fam in PLANE_FAMILIES:
        for mode in MODES:
            for cout in (64, 96, 160):  # 96: a partly filled last 64-column tile
                for tile in (hip.TILE_128x64_W4, None):
                    segs = [seg("c_none", 1, 6, 10, res=None, out="f32"), seg("c_f32", 2, 5, 7, filt=1, res="f32", out="planes"),
                            seg("c_pl", 1, 9, 15, res="planes", out="both"), seg("c_up", 1, 8, 12, filt=1, res="planes_up", out="planes"),
                            seg("c_f32b", 1, 1, 3, res="f32", out="both")]
                    out.append(launch(f"c_n{cout}", fam, mode, tile, 1 if tile is not None else None, segs, N=cout))
    return out


# ------------------------------------------------------------------------------------------------ group D
N_LIMITS = (3, 5, 20, 33, 55, 110)  # 33: one channel spills into the second 32-column block; 110 = 11 x 10 classes
D_LEVELS = [("l0", 1, 9, 15), ("l1", 2, 5, 7)]


def _d_segs(groups):
    # forward.py::_heads: every group (its own filter, zero-padded to the launch's N, and its own lo) at every level
    return [seg(f"{t}_n{nl}", B, H, W, filt=g, n_limit=nl, lo="mixed", out="f32") for g, nl in enumerate(groups) for t, B, H, W in D_LEVELS]


D_NARROW, D_WIDE = (3, 5, 20), (33, 55, 110, 5)


def group_d():
    """The predictor launches: n_limit per segment, per-channel lo, with and without the launch's relu (the test runs both).  Not covered,
    by design of ConvOp: n_limit with a split-plane output (ConvOp refuses it), and narrow (N <= 32) launches on the f32-input bf16x3
    kernel (ConvOp sends them to the f32 kernel)."""
    out = []
    mk = lambda fam, mode, tile, sk, groups: launch("d_narrow" if max(groups) <= 32 else "d_wide", fam, mode, tile, sk, _d_segs(groups),
                                                    N=max(groups), relu=False, data="bimodal")
    out.append(mk("f32", None, hip.TILE_128x32, 1, D_NARROW))
    for t in (hip.TILE_128x64, hip.TILE_128x128, None):
        out.append(mk("f32", None, t, 1 if t is not None else None, D_WIDE))
    for t in (hip.TILE_128x64, hip.TILE_256x128, None):
        out.append(mk("x3f32", None, t, 1 if t is not None else None, D_WIDE))
    for fam in PLANE_FAMILIES:
        for mode in MODES:
            out.append(mk(fam, mode, hip.TILE_128x32_W4, 1, D_NARROW))
            for t in (hip.TILE_128x64_W4, hip.TILE_256x128, None):
                out.append(mk(fam, mode, t, 1 if t is not None else None, D_WIDE))
    # split-K (Cin 64 = 18 K-tiles; 2 slices of 9: the row kernel stays)
    out.append(mk("f32", None, hip.TILE_128x64, 2, D_WIDE))
    out.append(mk("x3f32", None, hip.TILE_128x64, 2, D_WIDE))
    for fam in PLANE_FAMILIES:
        out.append(mk(fam, "f16x2", hip.TILE_128x64_W4, 2, D_WIDE))
        out.append(mk(fam, "bf16x3", hip.TILE_128x32_W4, 2, D_NARROW))
    return out


# ------------------------------------------------------------------------------------------------ group E
def group_e():
    """in_relu (p7 = conv(relu(p6))): the bf16x3 kernel on f32 input, 3 x 3 / stride 2 on odd maps and stride 1, one and two segments."""
    out = []
    for name, stride in (("e_s2", 2), ("e_s1", 1)):
        shapes = [("e0", 1, 13, 21), ("e1", 2, 5, 9)]
        for ns in (1, 2):
            out.append(launch(f"{name}_{ns}seg", "x3f32", None, None, None, [seg(t, B, H, W, filt=i) for i, (t, B, H, W) in enumerate(shapes[:ns])],
                              N=64, stride=stride, relu=False, in_relu=True, data="neg"))
    return out


# ------------------------------------------------------------------------------------------------ group F
F_RAISED = 5000.0  # x plane scale 16 = 80000 > 65504


def group_f_overflow():
    """[(baseline, raised)]: DD3D_MATH_F16X2, plane outputs, no clamp (relu 0, no lo).  The raised launch differs in ONE bias entry."""
    out = []
    for fam in PLANE_FAMILIES:
        for nm, ch, segs in (("f_ovf_c5", 5, [seg("f0", 1, 9, 15, out="both")]),
                             ("f_ovf_lastblock", 90, [seg("f0", 1, 9, 15, out="both"), seg("f1", 2, 5, 7, out="planes")])):  # 90: columns 64 .. 95 of N = 96
            mk = lambda rb: launch(nm, fam, "f16x2", hip.TILE_128x64_W4, 1, segs, N=96, relu=False, raise_bias=rb)
            out.append((mk(None), mk((0, ch, F_RAISED))))
    return out


def group_f_amax():
    """Launches whose stored values are all 1.5 (zero filters), so every reporting wave reports exactly 1.5 x plane scale."""
    z = dict(relu=False, data="zero_w")
    return [
        launch("f_amax_m3n5", "row", "f16x2", None, None, [seg("z0", 1, 1, 3, out="both")], N=5, **z),  # one, mostly empty, tile
        launch("f_amax_m3n5", "pertap", "f16x2", hip.TILE_64x64_W4, 1, [seg("z0", 1, 1, 3, out="both")], N=5, **z),
        # m65 / m385: the last tile holds ONE row, so the rotating reporting wave sits on rows >= M and must move to wave row 0
        launch("f_amax_multi", "row", "f16x2", hip.TILE_64x64_W4, 1, _a_segs(m_table(64), ("both", "planes")), **z),
        launch("f_amax_multi", "pertap", "f16x2", hip.TILE_128x64_W4, 1, _a_segs(m_table(128), ("both", "planes")), **z),
        launch("f_amax_sk", "row", "f16x2", hip.TILE_128x64_W4, 3, _a_segs(m_table(128), ("both", "planes")), Cin=96, **z),
        # entries fed by ONE tile whose rotating reporting wave holds no stored value (amax_feeders): rows >= M / columns >= N
        launch("f_amax_rowfb", "row", "f16x2", hip.TILE_64x64_W4, 1, _a_segs([("m65", 1, 5, 13), ("m3", 1, 1, 3)], ("both", "planes")), N=64, **z),
        launch("f_amax_colfb", "pertap", "f16x2", hip.TILE_64x64_W4, 1, _a_segs([("m65", 1, 5, 13), ("m3", 1, 1, 3)], ("planes", "both")), N=69, **z),
        launch("f_amax_randn", "row", "f16x2", hip.TILE_64x64_W4, 1, _a_segs(m_table(64), ("both", )), relu=False),  # real data: the bound only
    ]


def amax_slots(L, bm, bn):
    """The entries j of amax[32 j] a launch reports into: (m0 / BM + n0 / BN) & 15 over its tiles (csrc/conv_common.h::conv_epilogue_t)."""
    nn = -(-L["N"] // bn)
    return sorted({(mt + nt) & 15 for s in L["segs"] for mt in range(-(-seg_m(L, s) // bm)) for nt in range(nn)})


def amax_feeders(L, tile):
    """{entry j: [whether the tile's rotating reporting wave must be moved to wave row / column 0, per tile reporting into j]}."""
    from dd3d_amd.engine.tiling import TILE_WAVE_GRID
    tm, tn, wm, wn = TILE_WAVE_GRID[tile]
    bm, bn = tm * 32 * wm, tn * 32 * wn
    out = {}
    for s in L["segs"]:
        for mt in range(-(-seg_m(L, s) // bm)):
            for nt in range(-(-L["N"] // bn)):
                seed = mt + nt
                moved = mt * bm + (seed % wm) * tm * 32 >= seg_m(L, s) or nt * bn + ((seed // wm) % wn) * tn * 32 >= L["N"]
                out.setdefault(seed & 15, []).append(moved)
    return out


def all_launches():
    out = group_a() + group_c() + group_d() + group_e() + group_f_amax()
    for _, places in group_b():
        out += list(places.values())
    for base, raised in group_f_overflow():
        out += [base, raised]
    return out
