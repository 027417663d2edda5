"""CPU proof that tests/attention_ref.py has teeth: the arithmetic model of the flash-attention kernels stays well inside the
derived bound on every input family, each modelled kernel mistake breaks the bound on the family named for it, and the old
`randn` inputs are blind to a missing rescale of O^T on the MJ head dims (the reason the families exist)."""
import functools
import math

import pytest
import torch

import attention_ref as A

B, HEADS, SQ = 2, 3, 64
DIMS = (8, 40, 64, 80, 160)
ROUND = {"bf16": "bf16", "fp16": "fp16", "f16x3": "f16x3"}


@functools.lru_cache(maxsize=None)
def case(family, flavour, d, skv, causal=False, sq=SQ):
    q, k, v = A.make_inputs(family, B, HEADS, sq, skv, d, seed=1000 + 7 * d + skv, rnd=ROUND[flavour])
    ref = A.reference(q, k, v, HEADS, d ** -0.5, causal)
    bnd, bnd_lse = A.bound(q, k, v, HEADS, d ** -0.5, ref, flavour)
    return q, k, v, ref, bnd, bnd_lse


def ratios(family, flavour, d, skv, fault=None, causal=False, sq=SQ):
    q, k, v, ref, bnd, bnd_lse = case(family, flavour, d, skv, causal, sq)
    o, lse2 = A.emulate(q, k, v, HEADS, d ** -0.5, causal, flavour, fault=fault)
    return (o - ref[0]).abs() / bnd, (lse2 - ref[3]).abs() / bnd_lse, o


@pytest.mark.parametrize("skv", [77, 200])
@pytest.mark.parametrize("family", A.FAMILIES)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("flavour", A.FLAVOURS)
def test_correct_model_is_inside_the_bound(flavour, d, family, skv):
    r, r_lse, o = ratios(family, flavour, d, skv)
    assert not torch.isnan(o).any()
    print(f"model[{flavour}, d{d}, {family}, {SQ}x{skv}]: worst err/B {float(r.max()):.3f}, lse {float(r_lse.max()):.3f}")
    assert float(r.max()) <= 0.75
    assert float(r_lse.max()) <= 0.75


@pytest.mark.parametrize("family", ["peaked", "stairs_up", "forbidden"])
@pytest.mark.parametrize("d", [8, 64])
@pytest.mark.parametrize("flavour", A.FLAVOURS)
def test_correct_model_is_inside_the_bound_causal(flavour, d, family):
    r, r_lse, o = ratios(family, flavour, d, 77, causal=True, sq=77)
    assert not torch.isnan(o).any()
    assert float(r.max()) <= 0.75 and float(r_lse.max()) <= 0.75


def test_families_are_what_they_say():
    d, skv = 40, 200
    s = {f: case(f, "bf16", d, skv)[3][2] for f in A.FAMILIES}
    assert float(s["all_negative"].max()) < -10.0
    assert float(s["flat"].abs().max()) == 0.0
    assert float((case("flat", "bf16", d, skv)[3][3] - math.log2(skv)).abs().max()) < 1e-12      # l = skv
    # stairs: the tile maximum of a rising query climbs by about MJ_T exp2 units per tile, well over MJ_T over the row, and that of a
    # falling query drops as far: in a wave of both, the branch fires on lanes whose own offset has to stay
    for fam, rising in (("stairs_up", 0), ("stairs_down", 1)):
        tile_max = torch.stack([s[fam][..., t * 64: (t + 1) * 64].amax(-1) for t in range(4)], -1) * A.LOG2E
        up, down = tile_max[..., rising::2, :], tile_max[..., 1 - rising::2, :]
        assert float((up[..., 1:] - up[..., :-1]).median()) > 0.8 * A.MJ_T and float((up[..., 3] - up[..., 0]).min()) > A.MJ_T
        assert float((down[..., 3] - down[..., 0]).max()) < -A.MJ_T
    assert float(s["peaked"].abs().max()) > 15.0 and float(s["late_spike"].max()) > 10.0
    # forbidden: the masked key i + 1 is the hottest, key i the hottest visible one, and the answer is (close to) v_i
    q, k, v, ref, _, _ = case("forbidden", "bf16", 64, 77, True, 77)
    full = A.reference(q, k, v, HEADS, 64 ** -0.5, False)[2]
    i = torch.arange(76)
    assert bool((full[..., i, i + 1] > full[..., i, i] + 1.0).all())
    assert float(ref[1].diagonal(dim1=-2, dim2=-1).median()) > 0.9             # most rows: o_i = v_i to within the other keys' weight


# the families that must expose each fault (skv = 200: four tiles; the tail faults at 77; the causal one at S = 77)
FAULT_FAMILIES = {
    "no_o_rescale": ("stairs_up", "peaked"),
    "no_l_rescale": ("stairs_up", "peaked"),
    "drop_tile": ("dense", "flat"),
    "tail_unmasked": ("all_negative", "flat"),
    "offset_not_updated": ("stairs_up", "stairs_down"),
}


@pytest.mark.parametrize("d", [8, 40, 64, 80])
@pytest.mark.parametrize("flavour", A.FLAVOURS)
@pytest.mark.parametrize("fault", sorted(FAULT_FAMILIES))
def test_faults_are_caught(fault, flavour, d):
    skv = 77 if fault == "tail_unmasked" else 200
    for family in FAULT_FAMILIES[fault]:
        r, _, _ = ratios(family, flavour, d, skv, fault=fault)
        frac = float((~(r <= 1.0)).double().mean())                   # NaN counts as outside
        print(f"{fault}[{flavour}, d{d}, {family}]: {100 * frac:.1f} % of elements outside B, worst err/B {float(r.nan_to_num(1e30).max()):.3g}")
        assert frac >= 0.05, (fault, family, frac)


@pytest.mark.parametrize("d", [8, 64])
@pytest.mark.parametrize("flavour", A.FLAVOURS)
def test_causal_off_by_one_is_caught(flavour, d):
    for family in ("forbidden", "peaked"):
        r, _, _ = ratios(family, flavour, d, 77, fault="causal_off_by_one", causal=True, sq=77)
        frac = float((~(r <= 1.0)).double().mean())
        print(f"causal_off_by_one[{flavour}, d{d}, {family}]: {100 * frac:.1f} % outside B")
        assert frac >= 0.05, (family, frac)


@pytest.mark.parametrize("flavour", ["bf16", "fp16"])
def test_dense_inputs_are_blind_to_a_missing_rescale(flavour):
    """randn scores never exceed the first tile's maximum by MJ_T exp2 units, so the deferred-max branch never fires after tile 0:
    a d = 40 kernel that never rescaled O^T would pass every `randn` test.  stairs_up at the same shape does not let it through."""
    r, _, o = ratios("dense", flavour, 40, 200, fault="no_o_rescale")
    assert float(r.max()) <= 1.0
    assert torch.equal(o, ratios("dense", flavour, 40, 200)[2])
    assert float(ratios("stairs_up", flavour, 40, 200, fault="no_o_rescale")[0].max()) > 100.0
