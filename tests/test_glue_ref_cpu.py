"""CPU: the teeth of tests/test_glue_kernels_gpu.py.  For every kernel of tests/glue_ref.py the float32 restatement of the kernel's own
arithmetic lies within the derived bound of the float64 reference on EVERY case the GPU test runs -- so the reference and the bound agree
with a correct kernel --, and every mutant a kernel could turn into (an element dropped or counted twice, a skipped tail loop, the two k of
an MFMA step exchanged between the operands, `<` for `<=`, the last index on a tie, the mean of the cell at the image border,
align_corners=True, the -0.5 of the source coordinate missing, bf16 truncation, the background row of the next batch, `off` ignored) leaves
it on at least one of those cases.  The worst error / bound ratio per kernel is printed (profiles/glue_ref_ratios.txt keeps the table)."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glue_ref as G  # noqa: E402

RATIOS = {}


@torch.no_grad()
@pytest.mark.parametrize("name", list(G.KERNELS))
def test_fp32_restatement_stays_inside_the_bound_on_every_case(name):
    K = G.KERNELS[name]
    worst, amb, tot = 0.0, 0.0, 0
    for case in K.CASES:
        inp = K.inputs(case)
        ok, ratio = K.check(inp, K.emulate(inp))
        assert ok, (name, case, ratio)
        amb, tot = amb + inp.get("_ambiguous", (0, 0))[0], tot + inp.get("_ambiguous", (0, 0))[1]
        worst = max(worst, ratio)
    if tot:   # bf16 outputs: either neighbour is accepted on fewer than 1% of the elements
        assert amb / tot < G.AMBIGUOUS_SHARE, (name, amb / tot)
    if name == "bilinear_sample":
        assert worst <= G.BILINEAR_EMULATION_SHARE, worst
    RATIOS[name] = worst
    print("\n%-18s worst error / bound of the fp32 restatement: %.3f over %d cases" % (name, worst, len(K.CASES)))


def _cost(case):
    n = 1
    for v in case:
        if isinstance(v, int) and not isinstance(v, bool):
            n *= max(v, 1)
    return n


@torch.no_grad()
@pytest.mark.parametrize("name,mutant", [(n, m) for n, K in G.KERNELS.items() for m in K.MUTANTS])
def test_every_mutant_leaves_the_bound_on_a_gpu_case(name, mutant):
    """Cheapest cases first; on the case that catches the mutant the unmutated restatement passes."""
    K = G.KERNELS[name]
    for case in sorted(K.CASES, key=_cost)[:400]:
        inp = K.inputs(case)
        if not K.check(inp, K.emulate(inp, mutant))[0]:
            assert K.check(inp, K.emulate(inp))[0], (name, case)
            return
    raise AssertionError("%s: mutant %s passes every case" % (name, mutant))


def test_exact_inputs_are_exact_in_fp32():
    """The zero bounds: integer-valued operands sum exactly, and on the lattice the expansion |a|^2 - 2 a.b + |b|^2 is the squared distance."""
    for case in G.bmm.CASES:
        if case[6] == "int":
            inp = G.bmm.inputs(case)
            assert float(inp["A"].abs().max()) <= 8 and case[2] <= 512 and torch.equal(inp["A"], inp["A"].round())
    g = torch.Generator().manual_seed(1)
    a, b = G.lattice(2, 300, g), G.lattice(2, 513, g)
    assert torch.equal(a * 64, (a * 64).round()) and float(a.abs().max()) <= 1
    d2 = ((a[:, :, None].double() - b[:, None].double()) ** 2).sum(-1)
    e32 = ((a * a).sum(-1)[:, :, None] - 2 * torch.einsum("bik,bjk->bij", a, b)) + (b * b).sum(-1)[:, None, :]
    assert torch.equal(e32.double(), d2)
    inp = G.nearest_partner.inputs((300, 513, 1))
    dmin, arg, close = G.nearest_partner_64(inp["a"], inp["b"], 1, inp["thr"])
    d = G._nearest_dist64(inp["a"], inp["b"])
    assert bool((d == G.NEAREST_THR).any()), "the threshold is attained exactly"
    assert bool(((d == dmin[..., None]).sum(2) > 1).any()), "exact ties for the minimum"


def test_rne_interval_accepts_the_neighbour_only_at_a_boundary():
    ref = torch.tensor([1.0, 1.0 + 2.0 ** -8, 3.0], dtype=torch.float64)   # 1 + 2^-8: the midpoint of two bf16 values
    assert G.rne_ok(torch.tensor([1.0, 1.0, 3.0]), ref, 1e-7)[0] and G.rne_ok(torch.tensor([1.0, 1.0 + 2.0 ** -7, 3.0]), ref, 1e-7)[0]
    assert not G.rne_ok(torch.tensor([1.0 + 2.0 ** -7, 1.0, 3.0]), ref, 1e-7)[0]
    assert G.rne_ok(torch.tensor([1.0, 1.0, 3.0]), ref, 1e-7)[1] == pytest.approx(1 / 3)


def test_transpose_pad_bf16_refuses_a_batch_beyond_the_grid():
    """B goes on gridDim.y (at most 65535): refused before anything is launched, like the fp32 twin -- so this needs no device."""
    from unopose_amd._lib import call

    buf = (ctypes.c_float * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for name in ("unopose_transpose_pad_bf16", "unopose_transpose_pad_f32"):
        with pytest.raises(RuntimeError, match="bad shape"):
            call(name, p, 64, 65536, 2, 64, 2, p, None)


def test_zz_print_the_ratio_table():
    if RATIOS:
        print("\n" + G.ratio_table(RATIOS, "fp32 restatement (CPU)"))
