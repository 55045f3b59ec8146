"""CPU: the float64 reference of the ViT attention cores (tests/vit_attn_ref.py) against the package's composite and the oracle, the two
emulations of the kernels' declared arithmetic against the bounds, and the teeth of test_vit_attention_probes_gpu.py: every mutant a
kernel could turn into must leave the bound, by at least 4x on at least one element, on the probe family built for it.

All cases: B = 2, H = 2, T in 40 / 293 / 1057, seed 100 + T -- the cases vit_attn_ref.C32 was measured over."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vit_attn_ref as V  # noqa: E402

B, H = 2, 2
TS = (40, 293, 1057)
KINDS = ("bf16", "f32")
TEETH = 4.0


@functools.lru_cache(maxsize=None)
def case(family, T, kind):
    """(qkv, ref, A, bound) of one probe input; shared between the tests, never changed."""
    x = V.FAMILIES[family](B, T, H, 100 + T, bf16=kind == "bf16")
    ref, A = V.vit_attn_ref(x, H)
    return x, ref, A, (V.bf16_bound(A) if kind == "bf16" else V.f32_bound(x, H, A))


def caught(mutant, ref, bound):
    """The mutant's worst |mutant - ref| / bound."""
    return V.worst(mutant, ref, bound)[0]


# ------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("family", ["sharp", "match"])
@pytest.mark.parametrize("T", [40, 293])
def test_reference_equals_the_composite_and_the_oracle_in_float64(family, T):
    from oracle import unopose_ref as R
    from unopose_amd import ops

    x, ref, A, _ = case(family, T, "f32")
    scale = float(ref.abs().max())
    assert scale > 0.1 and bool((A >= ref.abs() * (1 - 1e-12)).all())
    for other in (ops.vit_attention_torch(x.double(), H), R.vit_attention_core(x.double(), H)):
        assert other.dtype == torch.float64 and float((other - ref).abs().max()) <= 1e-12 * scale


def test_split_layout_helpers_round_trip():
    x = V.sharp(1, 7, 1, 3).reshape(7, 192)
    s = V.to_split_layout(x)
    assert s.shape == (7, 384) and s.dtype == torch.bfloat16
    back = V.from_split_layout(s)
    assert float((back - x.double()).abs().max()) <= 2.0 ** -17 * float(x.abs().max())
    hi, lo = V.split_planes(x)
    assert torch.equal(s.reshape(7, 6, 2, 32)[:, :, 0].double().reshape(7, 192), hi)
    assert torch.equal(s.reshape(7, 6, 2, 32)[:, :, 1].double().reshape(7, 192), lo)


def test_families_are_what_they_say():
    T = 293
    # match: query t's largest weight is on key pi(t), and every key is owned once
    x, _, _, _ = case("match", T, "f32")
    q, k, _ = V.heads_of(x, H)
    top = (q @ k.transpose(-1, -2)).argmax(-1)
    assert torch.equal(top, V.match_owner(B, T, H, 100 + T))
    assert all(sorted(top[b, h].tolist()) == list(range(T)) for b in range(B) for h in range(H))
    # lastkey: every query's largest weight is on key T - 1, and it is most of the weight
    for kind in KINDS:
        q, k, _ = V.heads_of(case("lastkey", T, kind)[0], H)
        p = torch.softmax(q @ k.transpose(-1, -2) / 8, -1)
        assert float(p[..., T - 1].min()) > 0.9
    # stair: the tile maxima in the exp2 domain step by `step` +- 1
    for name, step in (("stair+9", 9), ("stair+5", 5), ("stair-9", -9)):
        for kind in KINDS:
            q, k, _ = V.heads_of(case(name, T, kind)[0], H)
            s2 = (q @ k.transpose(-1, -2)) * (V.LOG2E / 8)
            tiles = torch.stack([s2[..., a:a + 32].max(-1)[0] for a in range(0, T, 32)], -1)
            d = tiles[..., 1:] - tiles[..., :-1]
            assert float((d - step).abs().max()) < 1.0, (name, kind, float((d - step).abs().max()))
    # bait: what image 0's queries look for is in image 1's first rows, twice as large as any score inside image 0
    x = case("bait", T, "f32")[0]
    q, k, _ = V.heads_of(x, H)
    own = (q[0] @ k[0].transpose(-1, -2)).max(-1)[0]
    across = (q[0] @ k[1][:, :128].transpose(-1, -2)).max(-1)[0]
    assert bool((across > 1.9 * V.MAG_BAIT ** 2).all()) and bool((across > own + 8 * 8).all())
    back = (q[1] @ k[0][:, -128:].transpose(-1, -2)).max(-1)[0]
    assert bool((back > 1.9 * V.MAG_BAIT ** 2).all())


# ------------------------------------------------------------------------------------------------------ the emulations
@pytest.mark.parametrize("family", list(V.FAMILIES))
@pytest.mark.parametrize("T", TS)
def test_bf16_emulation_stays_inside_the_bf16_bound(family, T):
    x, ref, A, bound = case(family, T, "bf16")
    out = V.emulate_bf16(x, H, seed=T)
    assert bool(((out - ref).abs() <= bound).all()), V.describe(out, ref, bound)
    assert V.worst(out, ref, bound)[0] > 0.25   # ... and the bound is not slack: the emulation uses a good part of it


@pytest.mark.parametrize("family", list(V.FAMILIES))
@pytest.mark.parametrize("T", TS)
def test_f32x3_emulation_stays_inside_both_fp32_class_bounds(family, T):
    x, ref, A, _ = case(family, T, "f32")
    out = V.emulate_f32x3(x, H)
    hard = V.f32_hard_bound(x, H, A)
    assert bool(((out - ref).abs() <= hard).all()), V.describe(out, ref, hard)
    assert bool(((out - ref).abs() <= V.C32 * A).all()), V.describe(out, ref, V.C32 * A)


def test_c32_is_eight_times_the_emulations_worst():
    """C32 comes from the emulation over exactly these cases, not from a kernel: the literal must be 8 x the worst err / A (+ 2 % for
    the rounding of the literal)."""
    w = max(V.worst(V.emulate_f32x3(case(f, T, "f32")[0], H), case(f, T, "f32")[1], case(f, T, "f32")[2])[0]
            for f in V.FAMILIES for T in TS)
    assert 8 * w <= V.C32 <= 8 * w * 1.02, (w, V.C32)


# --------------------------------------------------------------------------------- mutants: dropped or unmasked key slots
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("family,T", [("match", 40), ("match", 293), ("match", 1057), ("sharp", 40), ("sharp", 293)])
def test_every_single_dropped_key_is_caught(family, T, kind):
    """`match`: at every T, every slot (T - 1 included) is the key of some query; `sharp`: up to T = 293 every key still carries
    enough weight for some query."""
    x, ref, A, bound = case(family, T, kind)
    r = V.drop_key_ratios(x, H, ref, bound)
    assert r.shape == (T,) and float(r.min()) >= TEETH, (int(r.argmin()), float(r.min()))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("family", ["lastkey", "match", "sharp"])
@pytest.mark.parametrize("T", TS)
def test_an_unmasked_duplicate_of_the_last_key_is_caught(family, T, kind):
    x, ref, A, bound = case(family, T, kind)
    assert caught(V.dup_last_key(x, H), ref, bound) >= TEETH
    if family == "lastkey":  # ... there it halves EVERY query's output
        m = V.dup_last_key(x, H)
        big = ref.abs() > 0.5 * A
        assert bool((((m - ref).abs() > 0.4 * ref.abs()) | ~big).all())


# ------------------------------------------------------------------------------------ mutants: misplaced V, head or image
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T", TS)
def test_two_swapped_v_rows_are_caught_on_match(T, kind):
    x, ref, A, bound = case("match", T, kind)
    for i in (0, T // 2, T - 2):
        assert caught(V.swap_v_rows(x, H, i), ref, bound) >= TEETH, i


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T", TS)
def test_swapped_heads_in_v_are_caught_on_match(T, kind):
    x, ref, A, bound = case("match", T, kind)
    assert caught(V.swap_v_heads(x, H, 0), ref, bound) >= TEETH


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T", TS)
def test_keys_read_from_the_next_image_are_caught_on_bait(T, kind):
    x, ref, A, bound = case("bait", T, kind)
    m = V.leak_next_image(x, H, 32)
    assert caught(m[:1], ref[:1], bound[:1]) >= TEETH
    assert torch.equal(m[1], V.vit_attn_ref(x[1:], H)[0][0])   # (the last image has no neighbour to read)


# ------------------------------------------------------------------------------------------------ mutant: the fix-up
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T", TS)
def test_an_unscaled_old_accumulator_is_caught_on_stair_plus_9(T, kind):
    x, ref, A, bound = case("stair+9", T, kind)
    assert caught(V.no_rescale(x, H), ref, bound) >= TEETH
    # the same mutant is the truth where the reference never moves after the first tile ...
    xd, refd, Ad, boundd = case("stair-9", T, kind)
    assert caught(V.no_rescale(xd, H), refd, boundd) < 1e-6


# ------------------------------------------------------------------------------------------- mutants: fp32-class terms
@pytest.mark.parametrize("T", TS)
def test_a_dropped_lo_term_is_caught_by_c32_on_sharp(T):
    """K lo . Q hi dropped in q k^T, and V's lo plane dropped: both stay under the hard bound's order of magnitude, both must be
    >= 4 x C32 * A somewhere."""
    x, ref, A, _ = case("sharp", T, "f32")
    sharp_bound = V.C32 * A
    assert caught(V.emulate_f32x3(x, H, drop_qk_lo=True), ref, sharp_bound) >= TEETH
    assert caught(V.emulate_f32x3(x, H, drop_v_lo=True), ref, sharp_bound) >= TEETH
    assert caught(V.emulate_f32x3(x, H), ref, sharp_bound) <= 1.0 / 8 + 1e-9
