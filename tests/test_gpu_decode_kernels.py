"""The decode attention and decode GEMM kernels, one launch at a time, against
float64 references on chosen shapes (tests/decode_ref.py states the contract,
the bound and the inputs; test_decode_ref.py checks the bound on the CPU).
Every case runs the f16 and the bf16 instantiation through one f16 context
(mwx_test_dec_attn / mwx_test_gemm_dec / mwx_test_gemm_dec_ex take the type
as a flag; the MX-fp8 weight kernels take their codes and scales directly)."""
import numpy as np
import pytest

import decode_ref as dr
import encoder_ref as er
import mwx

pytestmark = pytest.mark.gpu

TYPES = [pytest.param(False, id="f16"), pytest.param(True, id="bf16")]


@pytest.fixture(scope="module")
def ctx(make_model):
    c = mwx.Context.open(make_model("micro"))
    yield c
    c.close()


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint16 if x.dtype == np.float16 else np.uint32)


def launch(ctx, case, bf16, **kw):
    args = dict(bf16=bf16, active=case["active"], pos=case.get("pos"),
                kv_index=case.get("kv_index"), fixed_len=case.get("n", 0),
                qscale=case["qscale"], kscale=case["kscale"], scale=case["scale"])
    args.update(kw)
    return ctx.test_dec_attn(case["P"], case["bias"], case["kc"], case["vc"], **args)


def check_rows(o, rows, scale, bf16, active=None):
    """|o - o64| <= bound for every element of every active row; the worst ratio."""
    worst = 0.0
    for r, (q, K, V, *_) in enumerate(rows):
        if active is not None and not active[r]:
            continue
        assert np.isfinite(o[r]).all(), f"row {r}: non-finite output"
        o64, bound = dr.attention_ref(q, K, V, scale, bf16)
        ratio = np.abs(o[r].astype(np.float64) - o64) / bound
        assert ratio.max() <= 1.0, (f"row {r} (n = {len(K)}): |o - o64| / bound = {ratio.max():.3f} "
                                    f"at element {int(ratio.argmax())}")
        worst = max(worst, float(ratio.max()))
    return worst


def check_self_caches(case, rows, kc1, vc1, active=None):
    """The row appended at pos equals the reference bit for bit (active rows)
    and every other cache word is unchanged."""
    kexp, vexp = case["kc"].copy(), case["vc"].copy()
    kvi = case.get("kv_index")
    for r, (_, _, _, kn, vn) in enumerate(rows):
        if active is not None and not active[r]:
            continue
        slot = r if kvi is None else int(kvi[r])
        kexp[slot, :, case["pos"][r]] = kn
        vexp[slot, :, case["pos"][r]] = vn
    assert np.array_equal(bits(kc1), bits(kexp)), "K cache differs from the reference"
    assert np.array_equal(bits(vc1), bits(vexp)), "V cache differs from the reference"


# ----------------------------------------------------------- self-attention

@pytest.mark.parametrize("bf16", TYPES)
@pytest.mark.parametrize("KS", [1, 2, 5, 8])
@pytest.mark.parametrize("qs", [0.02, 3.0])
def test_self_attention_every_length(ctx, bf16, KS, qs):
    """One row per length 1 .. 448 (batch edges of 8 / 128 rows and the cap):
    outputs within the bound, the appended K / V bit-exact, no other cache word
    written, and no NaN taken from positions >= pos."""
    case = dr.self_case(0, qs, KS)
    rows = dr.self_rows(case)
    o, kc1, vc1 = launch(ctx, case, bf16)
    worst = check_rows(o, rows, case["scale"], bf16)
    check_self_caches(case, rows, kc1, vc1)
    print(f"self KS {KS} qs {qs}: worst |o - o64| / bound = {worst:.3f}")


@pytest.fixture(scope="module")
def beam_case():
    """Rows (pos, own_from) with own_from in {0, 1, mid, pos}. `contig`: every
    row's history in its own slot. `mapped`: positions below own_from live in
    two donor slots of the row (alternating), the row's own slot holds NaN
    there, and the unused map words are junk."""
    pairs = [(p, f) for p in (1, 37, 200, 447) for f in (0, 1, p // 2, p)]
    R, H, cap = len(pairs), 2, 448
    base = dr.self_case(1, 3.0, 5, H=H, lens=[p + 1 for p, _ in pairs], cap=cap)
    slots = 3 * R
    contig = dict(base)
    contig["kc"], contig["vc"] = dr.nan_cache(slots, H, cap), dr.nan_cache(slots, H, cap)
    contig["kc"][:R], contig["vc"][:R] = base["kc"], base["vc"]
    mapped = dict(contig)
    mapped["kc"], mapped["vc"] = contig["kc"].copy(), contig["vc"].copy()
    kvmap = np.full((R, cap), -7, np.int32)
    own_from = np.asarray([f for _, f in pairs], np.int32)
    for r, f in enumerate(own_from):
        for j in range(f):
            donor = R + 2 * r + (j & 1)
            kvmap[r, j] = donor
            for c in ("kc", "vc"):
                mapped[c][donor, :, j] = contig[c][r, :, j]
                mapped[c][r, :, j] = dr.nan_cache(1, H, 1)[0, :, 0]
    return contig, mapped, kvmap, own_from


@pytest.mark.parametrize("bf16", TYPES)
@pytest.mark.parametrize("map_row0", [0, 3])
def test_beam_position_map(ctx, beam_case, bf16, map_row0):
    """A history read through kvmap / own_from / map_row0 gives the bits of the
    same history lying contiguous in the row's own cache."""
    contig, mapped, kvmap, own_from = beam_case
    kvi = np.arange(len(own_from), dtype=np.int32)
    o0, k0, v0 = launch(ctx, contig, bf16, kv_index=kvi)
    km = np.where(kvmap >= 0, kvmap + map_row0, kvmap).astype(np.int32)
    o1, k1, v1 = launch(ctx, mapped, bf16, kv_index=kvi, kvmap=km, own_from=own_from,
                        map_row0=map_row0)
    rows = dr.self_rows(mapped, kvmap=km, own_from=own_from, map_row0=map_row0, kv_index=kvi)
    worst = check_rows(o1, rows, mapped["scale"], bf16)
    check_self_caches(dict(mapped, kv_index=kvi), rows, k1, v1)
    assert np.array_equal(bits(o1), bits(o0))
    print(f"beam map, map_row0 {map_row0}: worst ratio {worst:.3f}")


@pytest.mark.parametrize("bf16", TYPES)
@pytest.mark.parametrize("nq", [2, 5, 7])
def test_row_groups_equal_single_rows(ctx, bf16, nq):
    """The XCD-grouped 1-D grid (nq rows per clip, (R / nq) H = 12 groups: four
    early-exit workgroup windows) gives the bits of the (H, R) grid, for self
    and for cross attention."""
    H, R = 6, 2 * nq
    rng = np.random.default_rng(nq)
    lens = [int(x) for x in rng.integers(1, 130, R)]
    case = dr.self_case(2, 3.0, 4, H=H, lens=lens, cap=160)
    o1, k1, v1 = launch(ctx, case, bf16)
    og, kg, vg = launch(ctx, case, bf16, nq=nq)
    worst = check_rows(og, dr.self_rows(case), case["scale"], bf16)
    assert np.array_equal(bits(og), bits(o1))
    assert np.array_equal(bits(kg), bits(k1)) and np.array_equal(bits(vg), bits(v1))
    kvi = np.repeat(np.arange(2, dtype=np.int32), nq)
    xc = dr.cross_case(2, 257, R, H, 3, 2, kv_index=kvi, cap=257)
    x1, _, _ = launch(ctx, xc, bf16)
    xg, _, _ = launch(ctx, xc, bf16, nq=nq)
    worst = max(worst, check_rows(xg, dr.cross_rows(xc), xc["scale"], bf16))
    assert np.array_equal(bits(xg), bits(x1))
    print(f"row groups nq {nq}: worst ratio {worst:.3f}")


@pytest.mark.parametrize("bf16", TYPES)
@pytest.mark.parametrize("KS", [1, 8])
def test_prefill_append_equals_self_write(ctx, bf16, KS):
    """kv_append followed by write_new = 0 leaves the caches and the outputs
    of write_new = 1, bit for bit."""
    case = dr.self_case(3, 0.5, KS)
    o0, k0, v0 = launch(ctx, case, bf16)
    o1, k1, v1 = launch(ctx, case, bf16, prefill=True)
    assert np.array_equal(bits(o1), bits(o0))
    assert np.array_equal(bits(k1), bits(k0)) and np.array_equal(bits(v1), bits(v0))
    check_self_caches(case, dr.self_rows(case), k1, v1)


@pytest.mark.parametrize("bf16", TYPES)
@pytest.mark.parametrize("prefill", [False, True])
def test_inactive_rows_are_left_alone(ctx, bf16, prefill):
    """An inactive row writes neither its cache nor its output; the active
    rows give the bits of the all-active launch."""
    case = dr.self_case(4, 3.0, 2)
    rows = dr.self_rows(case)
    o_all, _, _ = launch(ctx, case, bf16, prefill=prefill)
    act = np.asarray([r % 3 != 1 for r in range(len(rows))], np.int32)
    o, k1, v1 = launch(ctx, case, bf16, active=act, prefill=prefill)
    check_self_caches(case, rows, k1, v1, active=act)
    on = act.astype(bool)
    assert np.array_equal(bits(o[on]), bits(o_all[on]))
    assert np.isnan(o[~on]).all()


# ---------------------------------------------------------- cross-attention

@pytest.mark.parametrize("bf16", TYPES)
@pytest.mark.parametrize("n", dr.CROSS_LENS)
def test_cross_attention_single_rows(ctx, bf16, n):
    """The run-time-count kernel at every tail (n % 16, odd batch counts, the
    1536-key limit) and, at 1500, the constant-count kernel under both load
    policies (R H n 256 bytes below and above 4 MB)."""
    KS = 1 + dr.CROSS_LENS.index(n) % 8
    case = dr.cross_case(0, n, 3, 2, KS, 3)
    o, k1, v1 = launch(ctx, case, bf16)
    worst = check_rows(o, dr.cross_rows(case), case["scale"], bf16)
    assert np.array_equal(bits(k1), bits(case["kc"])) and np.array_equal(bits(v1), bits(case["vc"]))
    if n == 1500:
        assert 3 * 2 * n * 256 <= 4 << 20 < 8 * 2 * n * 256
        big = dr.cross_case(1, n, 8, 2, KS, 2, kv_index=[0, 1, 1, 0, 0, 1, 0, 1])
        ob, _, _ = launch(ctx, big, bf16)
        worst = max(worst, check_rows(ob, dr.cross_rows(big), big["scale"], bf16))
    print(f"cross n {n} KS {KS}: worst ratio {worst:.3f}")


@pytest.mark.parametrize("bf16", TYPES)
@pytest.mark.parametrize("nq", [2, 3, 4, 5, 6, 7, 8])
def test_cross_attention_grouped_equals_single_rows(ctx, bf16, nq):
    """dec_xattn_kernel (f16 caches, nq rows per workgroup): within the bound
    and the single-row kernel's bits, at 1500 keys too (the run-time-count
    stream against the constant-count one). Group 1 mixes active and inactive
    rows."""
    R = 2 * nq
    kvi = np.repeat(np.asarray([1, 0], np.int32), nq)
    act = np.ones(R, np.int32)
    act[nq + 1::2] = 0
    on = act.astype(bool)
    worst = 0.0
    for n in (9, 257, 513, 1500, 1536):
        case = dr.cross_case(nq, n, R, 2, 1 + (n + nq) % 8, 2, kv_index=kvi)
        case["active"] = act
        o1, _, _ = launch(ctx, case, bf16)
        og, k1, v1 = launch(ctx, case, bf16, nq=nq, grouped=True)
        worst = max(worst, check_rows(og, dr.cross_rows(case), case["scale"], bf16, active=act))
        assert np.array_equal(bits(og[on]), bits(o1[on])), f"n = {n}"
        assert np.isnan(og[~on]).all() and np.isnan(o1[~on]).all()
        assert np.array_equal(bits(k1), bits(case["kc"]))
        assert np.array_equal(bits(v1), bits(case["vc"]))
    print(f"grouped cross nq {nq}: worst ratio {worst:.3f}")


def test_hooks_refuse_indices_outside_their_buffers(ctx):
    """No launch for an index the kernels would follow outside the buffers."""
    case = dr.self_case(0, 0.5, 2, lens=(3, 5), cap=8)
    ok = dict(bf16=False)
    launch(ctx, case, **ok)
    R, cap = 2, 8
    kvmap = np.zeros((R, cap), np.int32)
    bad = [dict(pos=np.asarray([2, cap], np.int32)),
           dict(pos=np.asarray([-1, 4], np.int32)),
           dict(kv_index=np.asarray([0, 2], np.int32)),
           dict(kv_index=np.asarray([-1, 0], np.int32)),
           dict(kvmap=kvmap, own_from=np.asarray([3, 0], np.int32)),            # own_from > pos
           dict(kvmap=kvmap + 2, own_from=np.asarray([1, 0], np.int32)),        # slot 2 of 2
           dict(kvmap=kvmap, own_from=np.asarray([1, 0], np.int32), map_row0=1),  # slot -1
           dict(own_from=np.asarray([0, 0], np.int32)),                         # no map
           dict(nq=3),                                                          # R % nq
           dict(grouped=True, nq=2)]                                            # self, grouped
    for kw in bad:
        with pytest.raises(ValueError):
            launch(ctx, case, **dict(ok, **kw))
    xc = dr.cross_case(0, 4, 2, 2, 1, 2, cap=8)
    launch(ctx, xc, **ok)
    for kw in (dict(fixed_len=9),                                               # > cap
               dict(grouped=True, nq=2, qscale=0.5),                            # no query scale
               dict(kvmap=kvmap, own_from=np.asarray([0, 0], np.int32)),        # cross, map
               dict(prefill=True)):                                             # cross, prefill
        with pytest.raises(ValueError):
            launch(ctx, xc, **dict(ok, **kw))
    with pytest.raises(ValueError):
        ctx.test_dec_attn(np.zeros((9, 2, 3 * 128), np.float32), case["bias"], case["kc"],
                          case["vc"], bf16=False, active=case["active"], pos=case["pos"])
    big = dr.nan_cache(1, 1, 1537)
    with pytest.raises(ValueError):
        ctx.test_dec_attn(np.zeros((1, 1, 64), np.float32), np.zeros(64, np.float32), big, big,
                          bf16=False, active=[1], fixed_len=1537)
    a, w = dr.gemm_inputs(0, 3, 16, 64)
    with pytest.raises(ValueError):
        ctx.test_gemm_dec(a[:, :48], w[:, :48], bf16=False, mode=1)


# --------------------------------------------------------------------- GEMM

GEMM_N = (16, 26, 80)
GEMM_M = (1, 5, 16, 17, 33, 64, 65, 100)
FULL_KS = (96, 384, 768, 1280, 1536, 2048, 3072, 4096, 5120)  # every k-steps-per-wave case


def both_shared(run):
    """run() with the shared-A kernels and with the per-strip grids."""
    prev = mwx.set_dec_shared(True)
    try:
        shared = run()
        mwx.set_dec_shared(False)
        return shared, run()
    finally:
        mwx.set_dec_shared(None if prev < 0 else bool(prev))


@pytest.mark.parametrize("bf16", TYPES)
@pytest.mark.parametrize("K", sorted(dr.SPLITK_KS))
def test_gemm_splitk_partials(ctx, bf16, K):
    """Every slab against the float64 product over its own K slice (1 to 5
    k-steps per wave, KS 1 / 4 / 5 / 8), the vocabulary's partial strip
    (N = 26), row tails, and above 64 rows the shared-A kernel's bits equal
    to the per-strip grid's."""
    KS = dr.SPLITK_KS[K]
    worst = 0.0
    for N in GEMM_N:
        for M in GEMM_M:
            a, w = dr.gemm_inputs(0, M, N, K)
            if M > 64:
                P, P2 = both_shared(lambda: ctx.test_gemm_dec(a, w, bf16=bf16, mode=0))
                assert np.array_equal(bits(P), bits(P2)), (M, N)
            else:
                P = ctx.test_gemm_dec(a, w, bf16=bf16, mode=0)
            assert P.shape == (KS, M, N)
            assert np.isfinite(P).all(), (M, N)
            for ks in range(KS):
                ref, bound = dr.gemm_ref(a, w, bf16, ks * K // KS, (ks + 1) * K // KS)
                ratio = np.abs(P[ks] - ref) / bound
                assert ratio.max() <= 1.0, (M, N, ks, float(ratio.max()))
                worst = max(worst, float(ratio.max()))
    print(f"split-K K {K} KS {KS}: worst |P - ref| / bound = {worst:.3f}")


@pytest.mark.parametrize("bf16", TYPES)
@pytest.mark.parametrize("K", FULL_KS)
def test_gemm_decode_full_k(ctx, bf16, K):
    """gemm_skinny at every k-steps-per-wave case of its K split (1, 2, 3, 4,
    6, 8, 10) and gemm_dec_shared above 64 rows, against float64."""
    worst = 0.0
    for N in GEMM_N:
        for M in GEMM_M:
            a, w = dr.gemm_inputs(1, M, N, K)
            if M > 64:
                c, c2 = both_shared(lambda: ctx.test_gemm_dec(a, w, bf16=bf16, mode=1))
                assert np.array_equal(bits(c), bits(c2)), (M, N)
            else:
                c = ctx.test_gemm_dec(a, w, bf16=bf16, mode=1)
            assert np.isfinite(c).all(), (M, N)
            ref, bound = dr.gemm_ref(a, w, bf16)
            ratio = np.abs(c - ref) / bound
            assert ratio.max() <= 1.0, (M, N, float(ratio.max()))
            worst = max(worst, float(ratio.max()))
    print(f"full-K K {K}: worst |c - ref| / bound = {worst:.3f}")


@pytest.mark.parametrize("bf16", TYPES)
def test_gemm_decode_residual_epilogue(ctx, bf16):
    """EPI_RES: (a.w + bias) + res, two more f32 roundings than EPI_F32."""
    worst = 0.0
    for K in (384, 1280):
        for M in (5, 100):
            a, w = dr.gemm_inputs(2, M, 26, K)
            rng = np.random.default_rng([K, M])
            bias = rng.standard_normal(26).astype(np.float32)
            res = rng.standard_normal((M, 26)).astype(np.float32)
            c = ctx.test_gemm_dec(a, w, bf16=bf16, mode=2, bias=bias, res=res)
            ref, bound = dr.gemm_ref(a, w, bf16)
            want = ref + bias[None] + res
            bound = bound + 2.0 ** -24 * (np.abs(ref + bias[None]) + np.abs(want))
            ratio = np.abs(c - want) / bound
            assert np.isfinite(c).all() and ratio.max() <= 1.0, (K, M, float(ratio.max()))
            worst = max(worst, float(ratio.max()))
    print(f"EPI_RES: worst ratio {worst:.3f}")


# ------------------------------ MX-fp8 weights, FFN1 epilogue, LayerNorm fold
# (mwx_test_gemm_dec_ex; the W8 kernels are bf16 only, as the engine runs them)

PACK_N = (64, 96, 160)
PACK_M = (1, 5, 17, 64, 65, 100)
LN_KS = (96, 384, 512, 768, 1024, 1280, 2048)   # 96: served by neither fold
MODEL_WIDTHS = (384, 512, 768, 1024, 1280)
KINDS = [pytest.param((False, False), id="f16"), pytest.param((True, False), id="bf16"),
         pytest.param((True, True), id="w8")]


@pytest.fixture(scope="module")
def gelu_tab(ctx):
    return ctx.test_gelu_table()


def same_bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()


def run_rows(M, run):
    """run() once; above 64 rows with the shared-A kernels and with the
    per-strip grids, which must give the same bits (every output of run())."""
    if M <= 64:
        return run()
    shared, strips = both_shared(run)
    one = isinstance(shared, np.ndarray)
    for x, y in zip((shared,) if one else shared, (strips,) if one else strips):
        assert same_bits(x, y), "shared-A and per-strip kernels differ"
    return shared


def widen16(u16, bf16):
    u16 = np.ascontiguousarray(u16, dtype=np.uint16)
    if bf16:
        return (u16.astype(np.uint32) << 16).view(np.float32)
    return u16.view(np.float16).astype(np.float32)


def weights(kind, seed, N, K, span=None):
    """(keywords of the weight operand, the values the kernel multiplies by):
    16-bit weights of std K^-1/2, or MX-fp8 codes and scales (span None: the
    MX encoding of those weights; else block exponents uniform over span)."""
    bf16, w8 = kind
    if not w8:
        w = dr.gemm_inputs(seed, 1, N, K)[1]
        return dict(w=w), dr.round_t(w, bf16)
    if span is None:
        codes, scales = er.mx_encode(dr.bf16_round(dr.gemm_inputs(seed, 1, N, K)[1]))
    else:
        codes, scales = dr.mx_dec_weights(seed, N, K, span)
    return dict(wq=codes, ws=scales), dr.mx_decode(codes, scales)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("K", [128, 512])
def test_w8_identity_probe(ctx, K, mode):
    """A = the K x K identity: output (k, n) (mode 0: of slab k // (K / KS)) is
    the bf16 widening of code[n][k] under scale[n][k / 32], bit for bit, and
    every other slab an exact 0: every (column, k) code position and every
    scale word of the partial-strip N = 26, all 254 finite codes, exponents
    -100 .. 100, through the per-strip and the shared-A kernels. (A code 0x00
    or 0x80 gives a zero of either sign: a sum that starts at +0 has no -0.
    Exponents whose products are bf16 subnormals or overflow are out of
    scope: they are no weight scale the loader's quantizer emits for bf16
    weights of a trained model, and bf16 MFMA inputs below 2^-126 are not
    pinned by the contract.)"""
    N, KS = 26, dr.SPLITK_KS[K] if mode == 0 else 1
    codes, scales = dr.mx_probe_weights(0, N, K)
    want = dr.mx_decode(codes, scales).T                       # [K][N]
    got = run_rows(K, lambda: ctx.test_gemm_dec_ex(np.eye(K, dtype=np.float32), bf16=True,
                                                   mode=mode, wq=codes, ws=scales))
    got = got.reshape(KS, K, N)
    exp = np.zeros((KS, K, N), np.float32)
    for ks in range(KS):
        rows = slice(ks * K // KS, (ks + 1) * K // KS)
        exp[ks, rows] = want[rows]
    nz = exp != 0
    bad = (nz & (bits(got) != bits(exp))) | (~nz & (got != 0))
    assert not bad.any(), (f"{int(bad.sum())} of {bad.size} words differ, first (slab, k, n) = "
                           f"{tuple(np.argwhere(bad)[0])}")


@pytest.fixture(scope="module")
def w8_runs(ctx):
    """(mode, K) -> the launches of the W8 kernels and of the bf16 16-bit
    kernels on the dequantised weights, made once for both tests below."""
    cache = {}

    def get(mode, K):
        if (mode, K) not in cache:
            out = []
            for N in (PACK_N if mode == 3 else GEMM_N):
                codes, scales = dr.mx_dec_weights(mode, N, K)      # exponents -30 .. 8
                w = dr.mx_decode(codes, scales)
                # mode 3: a times a power of two (exact) that brings the
                # pre-activations to a std of about 4, GELU's own range
                rms = np.sqrt((w.astype(np.float64) ** 2).sum(axis=1).mean())
                shrink = np.float32(2.0 ** -np.round(np.log2(rms / 4))) if mode == 3 else 1
                for M in GEMM_M:
                    a = dr.gemm_inputs(10 + mode, M, N, K)[0] * np.float32(shrink)
                    rng = np.random.default_rng([K, M, N])
                    bias = rng.standard_normal(N).astype(np.float32) if mode >= 2 else None
                    if mode == 3:
                        bias = np.linspace(-14.0, 14.0, N).astype(np.float32)
                    res = rng.standard_normal((M, N)).astype(np.float32) if mode == 2 else None
                    kw = dict(bf16=True, mode=mode, bias=bias, res=res)
                    g8 = run_rows(M, lambda: ctx.test_gemm_dec_ex(a, wq=codes, ws=scales, **kw))
                    g16 = run_rows(M, lambda: ctx.test_gemm_dec_ex(a, w, **kw))
                    out.append(dict(M=M, N=N, a=a, w=w, bias=bias, res=res, g8=g8, g16=g16))
            cache[mode, K] = out
        return cache[mode, K]
    return get


W8_CASES = [(0, K) for K in sorted(dr.SPLITK_KS)] + [(m, K) for m in (1, 2, 3) for K in FULL_KS]


@pytest.mark.parametrize("mode,K", W8_CASES)
def test_w8_equals_16bit_kernel_on_dequantised_weights(w8_runs, mode, K):
    """The contract above e8m0_to_f32: the codes are widened to bf16 exactly
    and the 16-bit MFMA chain runs unchanged, so the W8 kernels give the bits
    of the bf16 kernels on mx_decode(codes, scales): slabs, EPI_F32, EPI_RES
    and the packed EPI_GELU buffer, per-strip and shared-A (all four equal)."""
    for c in w8_runs(mode, K):
        g8, g16 = (c["g8"], c["g16"]) if mode == 3 else ((c["g8"],), (c["g16"],))
        for x, y in zip(g8, g16):
            assert same_bits(x, y), (c["M"], c["N"])


def gelu_packed_check(tab, got, a, w, bias, bf16):
    """The packed FFN1 output (c [M][N], the raw buffer): rows < M written and
    the pad rows untouched, the hook's unpacking = pack_index, every value a
    gelu_ggml output of an f16 input within the accumulator bound. Returns the
    float64 pre-activations."""
    c, raw = got
    M, N = c.shape
    ok, rows = dr.packed_store_ok(raw, M, N)
    assert ok, f"M {M} N {N}: a word of rows < M not written, or a pad row written"
    assert same_bits(widen16(rows, bf16), c)
    ref, beta = dr.gemm_ref(a, w, bf16)
    x64, bx = er.add_bound(ref, beta, bias.astype(np.float64)[None])
    okv = er.gelu_candidates_ok(c, x64, bx, tab, lambda g, sel: er.round_t(g, bf16))
    assert okv.all(), (f"M {M} N {N}: {(~okv).sum()} outputs are no GELU value of an f16 input "
                       f"within the bound, first at {np.argwhere(~okv)[0]}")
    return x64


@pytest.mark.parametrize("mode,K", W8_CASES)
def test_w8_against_float64(w8_runs, gelu_tab, mode, K):
    """The same launches against gemm_ref on the dequantised weights (exact in
    float64; the W operand has no rounding), the 16-bit tests' bound."""
    KS = dr.SPLITK_KS[K] if mode == 0 else 1
    worst = 0.0
    for c in w8_runs(mode, K):
        M, N, a, w, got = c["M"], c["N"], c["a"], c["w"], c["g8"]
        if mode == 3:
            gelu_packed_check(gelu_tab, got, a, w, c["bias"], True)
            continue
        assert got.shape == ((KS, M, N) if mode == 0 else (M, N)) and np.isfinite(got).all()
        for ks in range(KS):
            ref, bound = dr.gemm_ref(a, w, True, ks * K // KS, (ks + 1) * K // KS)
            want = ref
            if mode == 2:
                want = ref + c["bias"][None] + c["res"]
                bound = bound + 2.0 ** -24 * (np.abs(ref + c["bias"][None]) + np.abs(want))
            ratio = np.abs((got[ks] if mode == 0 else got) - want) / bound
            assert ratio.max() <= 1.0, (M, N, ks, float(ratio.max()))
            worst = max(worst, float(ratio.max()))
    print(f"W8 mode {mode} K {K}: " + ("every packed output a GELU value within the bound"
                                       if mode == 3 else
                                       f"worst |got - ref| / bound = {worst:.3f}"))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K", [128, 1280])
def test_gemm_decode_gelu_packed(ctx, gelu_tab, kind, K):
    """The decode FFN1 epilogue (EPI_GELU, pack_out) of gemm_skinny and, above
    64 rows, gemm_dec_shared (K 1280; equal bits): pre-activations spread over
    [-14, 14] by the bias (both saturation branches and everything between;
    over the case's launches at least 5 % beyond 10 and 5 % below 1), every
    output a gelu_ggml value (tanhf path) of an f16 input within the bound,
    stored at pack_index(m, n, N); rows M .. ceil64(M) - 1 keep the sentinel."""
    bf16, w8 = kind
    xs = []
    for N in PACK_N:
        kw, w = weights(kind, 20, N, K)
        bias = np.linspace(-14.0, 14.0, N).astype(np.float32)
        for M in PACK_M:
            a, _ = dr.gemm_inputs(21, M, N, K)
            got = run_rows(M, lambda: ctx.test_gemm_dec_ex(a, bf16=bf16, mode=3, bias=bias, **kw))
            xs.append(np.abs(gelu_packed_check(gelu_tab, got, a, w, bias, bf16)).reshape(-1))
    x = np.concatenate(xs)
    assert (x > 10).mean() >= 0.05 and (x < 1).mean() >= 0.05, ((x > 10).mean(), (x < 1).mean())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K", LN_KS)
def test_ln_fold_equals_two_launches(ctx, kind, K):
    """gemm_splitk_ln (the slabs) and gemm_decode_ln (the packed GELU output, N
    = 4 K capped at 4096) against layer_norm_dec followed by the plain GEMM, bit
    for bit, after 0 / 1 / 5 / 8 producer slabs: the outputs, x_out = that
    LayerNorm's residual, x_in unchanged, no guard band touched; an inactive
    row's x_out is a copy of x_in. A width is refused exactly where
    splitk_factor / skinny_split (with four waves) refuse it, and no model
    width is."""
    bf16, w8 = kind
    rng = np.random.default_rng(K)
    x = rng.standard_normal(K).astype(np.float32)
    lw = (1.0 + 0.5 * rng.standard_normal(K)).astype(np.float32)
    lb = (0.5 * rng.standard_normal(K)).astype(np.float32)
    Pall = rng.standard_normal((8, K)).astype(np.float32)
    pb = (0.3 * rng.standard_normal(K)).astype(np.float32)
    for mode, N in ((0, 90), (3, min(4 * K, 4096))):
        served = dr.ln_fold_serves(K, mode)
        assert served or K not in MODEL_WIDTHS, f"the fold does not serve model width {K}"
        kw, _ = weights(kind, 30, N, K, span=(-14, -10))
        kw.update(bf16=bf16, mode=mode,
                  bias=np.linspace(-14.0, 14.0, N).astype(np.float32) if mode == 3 else None)
        for KS in (0, 1, 5, 8):
            fuse = dict(x_in=x, w=lw, b=lb, active=1, P=Pall[:KS] if KS else None,
                        pbias=pb if KS else None)
            try:
                fold, x_out, x_after = ctx.test_gemm_dec_ex(ln=fuse, **kw)
            except NotImplementedError:
                assert not served, f"K {K} mode {mode}: the fold was lost"
                continue
            assert served, f"K {K} mode {mode}: served against the launcher's rule"
            y, x1 = ctx.test_layer_norm(x[None], lw, lb, bf16=bf16, dec=True,
                                        P=Pall[:KS, None] if KS else None, pbias=fuse["pbias"])
            two = ctx.test_gemm_dec_ex(y, **kw)
            for f, t in zip(*((fold, two) if mode == 3 else ((fold,), (two,)))):
                assert same_bits(f, t), (mode, KS)
            if mode == 3:
                assert dr.packed_store_ok(fold[1], 1, N)[0]
            assert same_bits(x_out, bits(x1[0])), (mode, KS, "x_out is not the residual")
            assert same_bits(bits(x_after), bits(x)), (mode, KS, "x_in changed")
        if served:
            fuse = dict(x_in=x, w=lw, b=lb, active=0, P=Pall[:5], pbias=pb)
            _, x_out, x_after = ctx.test_gemm_dec_ex(ln=fuse, **kw)
            assert same_bits(x_out, bits(x)) and same_bits(bits(x_after), bits(x)), mode


def test_gemm_dec_ex_refusals(ctx):
    """The hook's host checks: -1 (or -4 for a type the engine never runs)
    before any launch."""
    a, w = dr.gemm_inputs(0, 3, 64, 64)
    codes, scales = dr.mx_dec_weights(0, 64, 64)
    bias = np.zeros(64, np.float32)
    res = np.zeros((3, 64), np.float32)
    fuse = dict(x_in=a[0], w=a[1], b=a[2], active=1)
    ex = ctx.test_gemm_dec_ex
    ex(a, w, bf16=True, mode=3, bias=bias)
    ex(a, wq=codes, ws=scales, bf16=True, mode=2, res=res)
    bad = [dict(a=a[:, :48], w=w[:, :48], mode=1),                       # K % 32
           dict(a=a, w=w[:48], mode=3, bias=bias[:48]),                  # N % 32, packed
           dict(a=a[:2], w=w, mode=0, ln=fuse),                          # ln, M != 1
           dict(w=w, mode=1, ln=fuse),                                   # ln, mode 1
           dict(w=w, mode=0, ln=dict(fuse, P=np.zeros((9, 64), np.float32), pbias=bias)),  # KS 9
           dict(w=w, mode=0, ln=dict(fuse, P=np.zeros((2, 64), np.float32))),  # no pbias
           dict(w=w, mode=1),                                            # no a
           dict(a=a, wq=codes, mode=1),                                  # no scales
           dict(a=a, ws=scales, mode=1),                                 # no codes
           dict(a=a, w=w, mode=3),                                       # no bias, packed
           dict(a=a, w=w, mode=2),                                       # no residual
           dict(a=a, w=w, mode=1, bias=bias),                            # a bias EPI_F32 ignores
           dict(a=a, w=w, mode=4, bias=bias)]
    for kw in bad:
        with pytest.raises(ValueError):
            ex(kw.pop("a", None), kw.pop("w", None), bf16=True, **kw)
    with pytest.raises(NotImplementedError):                             # w8 is bf16 only
        ex(a, wq=codes, ws=scales, bf16=False, mode=1)
