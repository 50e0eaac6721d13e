"""The error table of tests/stats_conditioning.py, held on the CPU: for every family and input class the fp32 emulation of the
documented algorithm stays within C / 4 (in units of EPS32 * kappa_class), so no constant is set below what correct fp32
arithmetic needs; and where the conditioning is worst (the largest offset, the near-flat rows) the one-pass E[x^2] - mean^2
variant is at least ten times OUTSIDE C: the bound the GPU tests assert holds the right algorithm and rejects the wrong one."""
import pytest
import torch

from tests import stats_conditioning as S

CASES = [(f, n, d) for f in S.TABLE for n in S.family_classes(f) for d in S.EMU_WIDTHS[f]]


def test_table_is_complete():
    for fam, ent in S.TABLE.items():
        assert ent["C"] is not None and ent["emu"] is not None, fam
        assert 4 * ent["emu"] <= ent["C"] <= 8 * ent["emu"], fam          # four times the emulation; eight is the ceiling
        assert S.C[fam] == ent["C"]


@pytest.mark.parametrize("family,name,d", CASES)
def test_emulation_within_a_quarter_of_the_bound(family, name, d):
    r = S.emulation_ratio(family, name, d)
    assert r <= S.C[family] / 4, (family, name, d, r)


@pytest.mark.parametrize("name", [S.OFFSET_MAX, S.NEAR_FLAT])
@pytest.mark.parametrize("family,d", [(f, d) for f in S.TABLE for d in S.EMU_WIDTHS[f]])
def test_one_pass_variant_is_ten_times_outside(family, d, name):
    r = S.emulation_ratio(family, name, d, one_pass=True)
    assert r >= 10 * S.C[family], (family, name, d, r)


def test_kappa_and_classes():
    """kappa is what the module says, with eps inside rstd; the classes are what their names say; the interleave puts rows whose
    (mean, rstd) differ by orders of magnitude next to each other; the outlier changes its 32-column group from row to row."""
    x = torch.tensor([[1.0, 3.0], [5.0, 5.0]])
    k = S.kappa(x, 1e-5)
    assert abs(float(k[0]) - (1 + 4 / (1 + 1e-5)) ** 0.5) < 1e-12 and abs(float(k[1]) - (1 + 25 / 1e-5) ** 0.5) < 1e-6
    for name, lo, hi in (("offset+30", 25, 40), ("offset-300", 250, 400), ("offset+3000", 2500, 4000), ("flat7.3", 2300, 2320),
                         ("flat-1000", 3.1e5, 3.2e5), ("nearflat", 5000, 8000), ("commonsign", 1.5, 3), ("outlier", 1, 1.5)):
        km = float(S.kappa(S.make(name, 70, 512)).max())
        assert lo <= km <= hi, (name, km)
    assert float(S.kappa(S.make("flat0", 3, 32)).max()) == 1.0
    for rows in (70, 257):
        x = S.make("mixed", rows, 128)
        assert 5000 <= float(S.kappa(x).max()) <= 9000
        mu, _, rs = S.stats64(x)
        jump = (torch.log10(rs[1:] / rs[:-1]).abs() >= 0.8) | (torch.log10((mu[1:].abs() + 1e-30) / (mu[:-1].abs() + 1e-30)).abs() >= 0.8)
        assert float(jump.double().mean()) > 0.9
    o = S.make("outlier", 70, 512)
    col = (o == 200.0).double().argmax(-1)
    assert bool(((o == 200.0).sum(-1) == 1).all()) and bool((col[1:] // 32 != col[:-1] // 32).all())
    assert torch.equal(S.make("mixed", 70, 64, seed=3), S.make("mixed", 70, 64, seed=3))


def test_bn_columns_are_the_classes():
    v = S.bn_columns(400, S.BN_CLASSES)
    assert v.shape == (400, len(S.BN_CLASSES))
    for j, name in enumerate(S.BN_CLASSES):
        assert torch.equal(v[:, j], S.make(name, 1, 400, 300 + j)[0])
