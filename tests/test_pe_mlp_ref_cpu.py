"""CPU: the float64 reference of the PE neighbourhood MLP (tests/pe_mlp_ref.py) against the module chain, the bf16x3 emulation
against the reference's bound, and the teeth of test_pe_mlp_gpu.py: the mutants a kernel could turn into must leave the bound on the
inputs `make_case` builds."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pe_mlp_ref as P  # noqa: E402


@pytest.fixture(scope="module")
def case():
    """C = 200 centres, S = 64, with its reference and bound (shared, never changed)."""
    c = P.make_case(2, 100, 64, seed=3)
    c.ref, c.bound = P.pe_mlp_ref(c.pts, c.radius, c.lists, c.frames, c.folded)
    return c


def exceeds(c, out):
    return (out - c.ref).abs() > c.bound


def test_reference_equals_the_module_chain_in_float64():
    """An eval-mode _SharedMLP([6,32,64,128]) in double with non-trivial BatchNorm statistics (negative affine weight on every third
    channel), its Conv2d -> BatchNorm2d -> ReLU applied to the materialised (B,6,N,S) features, then max over S: pins
    _ConvBN.folded(), which feeds the reference here and the kernels in the package."""
    from unopose_amd.model.modules import _SharedMLP

    c = P.make_case(2, 9, 32, seed=5)
    torch.manual_seed(0)
    mlp = P.randomise_bn_(_SharedMLP([6, 32, 64, 128]), seed=1).double().eval()
    with torch.no_grad():
        folded = [l.folded() for l in mlp.layers()]
        assert all(w.dtype == torch.float64 for w, _ in folded)
        out, _ = P.pe_mlp_ref(c.pts, c.radius, c.lists, c.frames, folded)
        f, _ = P.features(c.pts, c.radius, c.lists, c.frames, 0, 18)
        x = f.reshape(2, 9, 32, 6).permute(0, 3, 1, 2)  # (B,6,N,S)
        for l in mlp.layers():
            assert not l.normlayer.bn.training
            x = torch.relu(l.normlayer.bn(l.conv(x)))
        chain = x.max(3)[0].permute(0, 2, 1)
    assert float(chain.max()) > 0.1
    assert float((out - chain).abs().max()) <= 1e-12 * float(chain.abs().max())
    # the independent float64 fold of the raw parameters agrees too
    for (w, b), (w2, b2) in zip(folded, P.fold64(mlp)):
        assert float((w - w2).abs().max()) <= 1e-14 * float(w.abs().max()) and float((b - b2).abs().max()) <= 1e-14 * float(b.abs().max())


def test_case_is_what_it_says(case):
    c = case
    S = c.S
    ids = c.lists.long() & 0xFFFF
    cnt = c.counts.long()
    assert sorted(set(cnt.flatten().tolist())) == [-1, 0, 1, 2, 31, 32, 33, 63, 64]
    far = torch.stack([torch.cdist(p, p).argmax(1) for p in c.pts.double()])
    for b in range(ids.shape[0]):
        for n in range(ids.shape[1]):
            k, row = int(cnt[b, n]), ids[b, n]
            if k == -1:
                assert len(set(row.tolist())) == S
            elif k == 0:
                assert bool((row == 0).all())
            else:
                assert bool((row[k:] == row[0]).all())
                assert len(set(row[:k].tolist())) == k
                if k > 1:
                    assert int(row[k - 1]) == int(far[b, n])
    assert bool((c.ref[:, :, c.dead] == 0).all()) and float(c.ref.max()) > 1.0


def test_bf16x3_emulation_stays_within_the_bound(case):
    c = case
    emu = P.bf16x3_emulated(c.pts, c.radius, c.lists, c.frames, c.folded)
    ratio = ((emu - c.ref).abs() / c.bound.clamp_min(1e-300)).max().item()
    print(f"bf16x3 emulation: worst err / bound = {ratio:.4f}")
    assert not exceeds(c, emu).any(), ratio
    assert bool((emu[:, :, c.dead] == 0).all())


def test_bound_is_small_against_the_output(case):
    assert float(case.bound.max()) <= 1e-3 * float(case.ref.max()), (float(case.bound.max()), float(case.ref.max()))


@pytest.mark.parametrize("layer", [0, 1, 2])
def test_hi_only_mutant_leaves_the_bound(case, layer):
    """One layer's weights without their lo part: at least 1 % of the output elements leave the bound."""
    c = case
    out = P.pe_mlp_values(c.pts, c.radius, c.lists, c.frames, P.hi_only(c.folded, layer))
    share = exceeds(c, out).float().mean().item()
    print(f"hi_only({layer}): {share:.2%} of the elements outside the bound")
    assert share >= 0.01, share


def test_drop_last_tile_mutant_leaves_the_bound_at_every_centre_it_touches(case):
    c = case
    out = P.drop_last_tile(c.pts, c.radius, c.lists, c.counts, c.frames, c.folded)
    hit = exceeds(c, out).any(2)
    touched = P.dropped_centres(c.counts, c.S)
    assert int(touched.sum()) >= 60
    assert bool(hit[touched].all()), int((~hit[touched]).sum())


@pytest.mark.parametrize("mutant", ["in", "out"])
def test_permutation_mutants_leave_the_bound(case, mutant):
    """Input channels 4 and 8 of layer 2 swapped; output rows 4 and 8 of layer 3 swapped: the moves pe_kperm and cd_row make."""
    c = case
    folded = P.swap_in(c.folded, 1, 4, 8) if mutant == "in" else P.swap_out(c.folded, 2, 4, 8)
    out = P.pe_mlp_values(c.pts, c.radius, c.lists, c.frames, folded)
    bad = exceeds(c, out)
    print(f"swap_{mutant}: outside the bound at {bad.any(2).float().mean().item():.1%} of the centres")
    assert bad.any()
    assert bad.any(2).float().mean().item() >= 0.5  # (a permuted kernel is wrong wherever the two channels differ, not at one odd centre)
