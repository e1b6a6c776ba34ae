"""kiss_hip_ctx_verify_sa_dev against its host model (tests/verify_model.py), mutation by mutation: every family of
tests/verify_mutations.py planted into a correct suffix array, the whole report compared field by field (equality of
integers; order_violations / first_violation only where they are a function of the input, see the model's docstring),
the text passed at every byte alignment, faults planted beyond the reach of the first grid-stride visit of the
permutation kernel (entries past 256 * 64 * 256 = 4 194 304), and a seeded randomised block."""
import numpy as np
import pytest

from tests import gen, verify_model, verify_mutations as vm
from tests.test_suffix_sort_gpu import _random_text

pytestmark = pytest.mark.gpu

K_UNBOUNDED = verify_model.K_UNBOUNDED
FIRST_VISIT = 256 * 64 * 256  # entries the permutation kernel reaches in the first pass of its grid-stride loop


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ctx():
    import kiss_amd
    c = kiss_amd.Context(max_n=20_000_000, device=0)
    yield c
    c.close()


def upload_text(torch_dev, S, offset=0):
    """the text on the device, `offset` bytes into a larger allocation: (tensor to keep alive, pointer to the text)"""
    torch, dev = torch_dev
    host = np.full(S.size + offset + 16, 0xA5, np.uint8)  # what surrounds the text is neither 0 nor a text byte
    host[offset:offset + S.size] = S
    buf = torch.from_numpy(host).to(dev)
    assert buf.data_ptr() % 8 == 0
    return buf, (buf.data_ptr() + offset if S.size else 0)


def dev_report(ctx, torch_dev, S, SA, k, offset=0, text=None):
    torch, dev = torch_dev
    buf, ptr = text if text is not None else upload_text(torch_dev, S, offset)
    d_SA = torch.from_numpy(np.ascontiguousarray(SA, dtype=np.uint32).view(np.int32)).to(dev)
    torch.cuda.synchronize()
    return ctx.verify_sa_dev(ptr, S.size, d_SA.data_ptr(), k)


def check_case(ctx, torch_dev, case, label, offsets=(0,), model=None):
    model = model or verify_model.report(case.S, case.SA, case.k)
    for offset in offsets:
        rep = dev_report(ctx, torch_dev, case.S, case.SA, case.k, offset)
        assert not verify_model.mismatches(rep, model), (label, offset, verify_model.mismatches(rep, model), rep)
        for field, value in case.what_must_hold.items():
            assert rep[field] == value or model[field] is None, (label, offset, field, value, rep)
    return model


@pytest.mark.parametrize("family", vm.FAMILIES)
def test_family_against_the_model(ctx, torch_dev, oracle, family):
    for label, case in vm.cases(family, oracle.suffix_sort, _random_text):
        if family.startswith("depth"):
            # the text at every alignment; and the unswapped array, which must pass with the same counts of ties
            check_case(ctx, torch_dev, case, label, offsets=range(8))
            i, j = case.touched
            good = vm.Case(case.S, vm.swapped(case.SA, i, j), case.k, (), {"ok": 1, "order_violations": 0})
            check_case(ctx, torch_dev, good, label + " unswapped", offsets=(0, 3))
        else:
            check_case(ctx, torch_dev, case, label, offsets=(0, 5) if case.S.size else (0,))


def test_first_entry_out_of_range_is_not_the_sentinel(ctx, torch_dev):
    """regression: SA[0] > n took the out-of-range exit of the permutation kernel before SA[0] was compared with n, and
    the report said sa0_ok = 1 (ok was 0 through out_of_range; no accepted array was affected)"""
    S = gen.iid(1000, 1)
    SA = vm.naive_sa(S)
    for k in (32, K_UNBOUNDED):
        for value in (S.size + 1, 0xFFFFFFFF):
            bad = SA.copy()
            bad[0] = value
            rep = dev_report(ctx, torch_dev, S, bad, k)
            assert (rep["sa0_ok"], rep["out_of_range"], rep["duplicates"], rep["ok"]) == (0, 1, 0, 0), (k, value, rep)


@pytest.fixture(scope="module")
def random_block(oracle):
    out = []
    for block in range(vm.RANDOM_BLOCKS):
        rng = np.random.default_rng(vm.RANDOM_SEED + block)
        for _ in range(vm.RANDOM_CASES_PER_BLOCK):
            case = vm.random_case(rng, oracle.suffix_sort, _random_text)
            out.append((case, verify_model.report(case.S, case.SA, case.k)))
    return out


def test_randomised_block_meets_its_shares(random_block):
    sh = vm.shares([m for _, m in random_block])
    print("randomised block:", sh)
    vm.check_shares(sh)


@pytest.mark.parametrize("block", range(vm.RANDOM_BLOCKS))
def test_randomised_block(ctx, torch_dev, random_block, block):
    per = vm.RANDOM_CASES_PER_BLOCK
    for c, (case, model) in enumerate(random_block[block * per:(block + 1) * per]):
        label = "block %d case %d: n=%d k=%d touched=%s text=%s..." % (block, c, case.S.size, case.k, case.touched[:8],
                                                                     case.S[:40].tolist())
        check_case(ctx, torch_dev, case, label, offsets=(int(c % 8),), model=model)


# ---- beyond the first grid-stride visit --------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[5_000_000, 20_000_000])
def large(request, ctx, torch_dev):
    n = request.param
    S = gen.genome_like(n, 21) if n == 5_000_000 else gen.iid(n, 22)
    SA = ctx.suffix_sort(S, K_UNBOUNDED)
    assert verify_model.is_suffix_array(S, SA)  # the model's proof, before anything is derived from this array
    text = upload_text(torch_dev, S)
    base = {k: dev_report(ctx, torch_dev, S, SA, k, text=text) for k in (256, K_UNBOUNDED)}
    for k, rep in base.items():
        assert not verify_model.mismatches(rep, verify_model.report_near(S, SA, k, ()), FIELDS_NOT_TIED), (k, rep)
        assert rep["ok"] == 1
    return S, SA, text, base


FIELDS_NOT_TIED = [f for f in verify_model.FIELDS if f != "tied_pairs"]


def check_large(ctx, torch_dev, large, case, label):
    S, SA, text, base = large
    assert case.touched and min(t for t in case.touched if t) > FIRST_VISIT, "the fault is not where this test wants it"
    rep = dev_report(ctx, torch_dev, S, case.SA, case.k, text=text)
    model = verify_model.report_near(S, case.SA, case.k, case.touched)
    fields = [f for f in FIELDS_NOT_TIED if model[f] is not None]
    assert not verify_model.mismatches(rep, model, fields), (label, verify_model.mismatches(rep, model, fields), rep)
    for field, value in case.what_must_hold.items():
        assert rep[field] == value or model[field] is None, (label, field, value, rep)
    # ties: the device's count moves by what the touched pairs contribute
    before = verify_model.report_near(S, SA, case.k, case.touched)["tied_pairs"] if case.k < S.size else 0
    assert rep["tied_pairs"] - base[case.k]["tied_pairs"] == model["tied_pairs"] - before, (label, rep, model, before)


def far_cases(S, SA, k, rng):
    """(label, Case): each fault alone, every index beyond FIRST_VISIT (index 0 where the sentinel is concerned)"""
    n = S.size
    far = lambda m: [int(v) for v in rng.choice(np.arange(FIRST_VISIT + 1, n + 1), m, replace=False)]
    yield "SA[0] <-> far", vm.sentinel_swap(S, SA, k, far(1)[0])
    yield "n twice", vm.sentinel_twice(S, SA, k, far(1)[0])
    idx = far(2)
    yield "one duplicate", vm.duplicate_values(S, SA, k, idx[0], idx[1:])
    idx = far(6)
    yield "six copies", vm.duplicate_values(S, SA, k, idx[0], idx[1:])
    yield "one out of range", vm.out_of_range_values(S, SA, k, far(1), [n + 1])
    yield "four out of range", vm.out_of_range_values(S, SA, k, far(4), [n + 1, 0xFFFFFFFF, n + 1, 0x80000000])
    i = far(1)[0]
    yield "adjacent swap at %d" % i, vm.adjacent_swap(S, SA, k, i)
    yield "adjacent swap at n", vm.adjacent_swap(S, SA, k, n)


def together(S, SA, k, rng):
    n = S.size
    idx = [int(v) for v in FIRST_VISIT + 1 + rng.choice((n - FIRST_VISIT) // 4 - 2, 12, replace=False) * 4]  # 4 apart
    return vm.compose(vm.sentinel_twice(S, SA, k, idx[0]), vm.duplicate_values(S, SA, k, idx[1], idx[2:5]),
                      vm.out_of_range_values(S, SA, k, idx[5:8], [n + 1, 0xFFFFFFFF, n + 2]),
                      vm.adjacent_swap(S, SA, k, idx[8] + 1), vm.far_swap(S, SA, k, idx[9], idx[10]))


@pytest.mark.parametrize("k", [256, K_UNBOUNDED])
def test_faults_beyond_the_first_grid_stride_visit(ctx, torch_dev, large, k):
    S, SA = large[:2]
    rng = np.random.default_rng(S.size + (k & 0xFFFF))
    if S.size == 5_000_000:  # one per run
        for label, case in far_cases(S, SA, k, rng):
            check_large(ctx, torch_dev, large, case, "n=%d k=%d %s" % (S.size, k, label))
    else:  # 20 M: five visits per thread; the swap and everything at once (the host model takes seconds per case here)
        n = S.size
        last_visit = int(rng.integers(4 * FIRST_VISIT + 1, n))
        check_large(ctx, torch_dev, large, vm.adjacent_swap(S, SA, k, last_visit), "n=%d k=%d swap at %d" % (n, k, last_visit))
        idx = [int(v) for v in rng.integers(4 * FIRST_VISIT + 1, n, 2)]
        assert idx[0] != idx[1]
        check_large(ctx, torch_dev, large, vm.duplicate_values(S, SA, k, idx[0], idx[1:]), "n=%d k=%d duplicate" % (n, k))
    case = together(S, SA, k, rng)
    assert case.what_must_hold == {"ok": 0, "duplicates": 4, "out_of_range": 3, "sa0_ok": 1}
    check_large(ctx, torch_dev, large, case, "n=%d k=%d all together" % (S.size, k))

