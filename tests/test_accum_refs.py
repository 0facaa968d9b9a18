"""The integer models of tests/accum_cases.py against plain big-integer arithmetic (no GPU): for every
new or changed function on the mixed-addition path (the joined reduction, the seeded lockstep pairs,
the symmetric squares, the prepared-operand products) and every directed operand, the model's words are
normalized limbs of a value below 2p that is congruent to the textbook result, every column stays
inside the bound its header comment states (the models assert those on the way), the three ways the
Montgomery scan can take its carry give the same words, and the symmetric square's columns are the
full product's."""
import pytest

import accum_cases as ac
import field_cases as fc

P = fc.P
SUITES = ac.suites()


def _val(e):
    return tuple(fc.val29(x) for x in e)


def _want(name, c):
    """per lane, the value the words must be congruent to (before the division by R)"""
    v = fc.val29
    if name == "f29_sqr_x2":
        return (v(c[0]) ** 2, v(c[1]) ** 2) * 2
    if name == "f29_mul_x2":
        return (v(c[0]) * v(c[1]), v(c[2]) * v(c[3]))
    if name == "f29_mul2_x2":
        return (v(c[0]) * v(c[1]) + v(c[2]) * v(c[3]), v(c[4]) * v(c[5]) + v(c[6]) * v(c[7]))
    if name == "pair_mul_x2":
        return fc.f2_mul(_val(c[0]), _val(c[1])), fc.f2_mul(_val(c[2]), _val(c[3]))
    if name == "pair_sqr_x2<16,8>":
        return fc.f2_mul(_val(c[0]), _val(c[0])), fc.f2_mul(_val(c[1]), _val(c[1]))
    if name == "f29_mul":
        return (v(c[0]) * v(c[1]),)
    if name == "f29_mul2":
        return (v(c[0]) * v(c[1]) + v(c[2]) * v(c[3]),)
    if name == "f29_redc_sum4":
        return (sum(v(c[2 * i]) * v(c[2 * i + 1]) for i in range(4)),)
    if name == "pair_mul":
        return fc.f2_mul(_val(c[0]), _val(c[1]))
    if name == "pair_mul_sum":
        x, y = fc.f2_mul(_val(c[0]), _val(c[1])), fc.f2_mul(_val(c[2]), _val(c[3]))
        return (x[0] + y[0], x[1] + y[1])
    return fc.f2_mul(_val(c[0]), _val(c[0]))  # pair_sqr_b<KB>


@pytest.mark.parametrize("name", [n for n in SUITES if n != "pair_prep"])
def test_model_words_bound_and_congruence(name):
    cases, lanes, model = SUITES[name]
    assert len(cases) >= 500
    for c in cases:
        out = model(c)
        assert len(out) == lanes
        want = _want(name, c)
        for lane, words in enumerate(out):
            # a lane's output: one result, or the results of a lockstep pair one after the other
            parts = [words[i:i + 14] for i in range(0, len(words), 14)]
            if lanes == 1:
                wants = want
            else:  # Fq2: coefficient `lane` of each result
                wants = [w[lane] for w in (want if len(parts) > 1 else (want,))]
            assert len(parts) == len(wants), name
            for w, x in zip(parts, wants):
                assert fc.normalized(w), (name, c)
                val = fc.val29(w)
                assert val < 2 * P, (name, c)
                assert (val - x * ac.R29I) % P == 0, (name, c)


def test_directed_operands_are_present():
    """all limbs 2^29 - 1, limbs 2^30 - 2 after doubling, K p - 1 and K p + 1, loose X < 8p and Y < 4p"""
    sq = [c[0] for c in SUITES["f29_sqr_x2"][0]]
    assert any(all(x == fc.M29 for x in a[:13]) for a in sq)  # doubled: 2^30 - 2 in every column
    vals = {fc.val29(a) for a in sq}
    for k in (1, 2, 4, 8):
        assert k * P - 1 in vals and k * P + 1 in vals, k
    assert 16 * P - 1 in vals
    mul = SUITES["f29_mul"][0]
    assert any(max(b) == (1 << 30) - 1 for _, b in mul) and any(max(b) == (1 << 30) - 2 for _, b in mul)
    pm = SUITES["pair_mul"][0]
    assert any(fc.val29(a[0]) == 10 * P - 1 for a, _ in pm) and any(fc.val29(b[1]) == 8 * P - 1 for _, b in pm)
    xs = {fc.val29(e[0][0]) for e in SUITES["pair_sqr_b<16>"][0]} | {fc.val29(e[0][1]) for e in SUITES["pair_sqr_b<16>"][0]}
    assert {8 * P - 1, 4 * P - 1, 4 * P + 1, 8 * P + 1} <= xs


@pytest.mark.parametrize("name", ["f29_sqr_x2", "f29_mul", "f29_mul2"])
def test_carry_forms_agree(name):
    """joined, seeded and split scans: the same words, each inside 2^64 at every partial sum"""
    for c in SUITES[name][0][::3]:
        cols = ac.sqr_columns(c[0]) if name == "f29_sqr_x2" else ac.columns([c[i:i + 2] for i in range(0, len(c), 2)])
        want = ac.redc(cols, form="joined")
        assert ac.redc(cols, form="seeded") == want and ac.redc(cols, form="split") == want


def test_redc4_carry_forms_agree():
    for c in SUITES["f29_redc_sum4"][0][::3]:
        pr = [c[0:2], c[2:4], c[4:6], c[6:8]]
        assert ac.redc4(pr, "seeded") == ac.redc4(pr, "joined")


def test_symmetric_square_columns_are_the_full_products():
    for a, _ in SUITES["f29_sqr_x2"][0]:
        assert ac.sqr_columns(a) == ac.columns([(a, a)])


def test_prepared_operands():
    """one exchange and selects give what the quad-permutes gave: y1 = b0 on both lanes; y2 = 16p - b1
    limb by limb in [0, 2^30) on the even lane, b1 on the odd one"""
    for (b,) in SUITES["pair_prep"][0]:
        (e1, e2), (o1, o2) = ac.prep(*b)
        assert e1 == o1 == tuple(b[0]) and o2 == tuple(b[1])
        assert fc.val29(e2) == 16 * P - fc.val29(b[1])
        assert fc.normalized(e1) and fc.normalized(o2)  # only the even lane's y2 carries 2^30 limbs
