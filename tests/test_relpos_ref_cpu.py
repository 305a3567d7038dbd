"""tests/relpos_ref.py checked without a GPU: hip.relpos_pairs on CPU tensors against the pair-list checker on every bucket case and its
cache behaviour; the fp32 re-statement of op_relpos_bias_bwd against fp64 (equal on the `int` family, inside E_r on `real`: the largest
share is printed); every mutant of the re-statement rejected by the `int`-equality gate AND by the bit comparison; the references
against the oracle's formulas; and relpos.joint_handle's bucket and id assembly with ops.RelPosBias stubbed (nothing is launched)."""
import pytest
import torch

from oracle import onepeace_oracle as O
from tests import relpos_ref as R

I32 = torch.int32


def hipmod():
    from one_peace_amd import hip
    return hip


def lists_of(case):
    """hip.relpos_pairs on a private CPU copy of the case's bucket (a view stays a view: the same strides)."""
    hip = hipmod()
    b = case.bucket
    if not b.is_contiguous():
        full = torch.zeros(b.stride(0), b.stride(0), dtype=I32)
        full[:case.S, :case.S] = b
        b = full[:case.S, :case.S]
    else:
        b = b.clone()
    return hip.relpos_pairs(b, case.S, case.num_rel)


def test_mirrors():
    hip = hipmod()
    assert R.PAIR_SEG == hip.PAIR_SEG
    assert all(R.attn_spad(S) == hip.attn_spad(S) for S in (1, 17, 128, 129, 257, 1025))
    # the grid-stride routes that the GPU test claims to reach
    assert R.trips(1025 * 1152) > 1 and R.trips(5 * 300 * 384) > 1 and R.trips(5 * 2 * 300 * 300) > 1
    c = R.bucket_case("image32")
    assert c.num_rel == 3972 and R.trips((c.S * c.S // R.PAIR_SEG + c.num_rel) * 16) > 1
    assert R.trips(c.num_rel * 24) == 1      # relpos_seg_fold_kernel stays inside one trip (see the module docstring)


def test_table_values_are_distinct():
    t = R.make_table(514, 24)
    assert bool(torch.isfinite(t.float()).all()) and t.view(torch.int16).unique().numel() == 514 * 24
    big = R.make_table(3972, 24).view(torch.int16)      # past P entries: rows of one head and heads of one row still differ
    assert all(big[:, h].unique().numel() == 3972 for h in (0, 23))
    assert int((big.sort(1).values.diff(dim=1) == 0).sum()) == 0


@pytest.mark.parametrize("name", R.BUCKET_NAMES)
def test_pair_lists(name):
    c = R.bucket_case(name)
    lists = lists_of(c)
    assert R.check_pairs(lists, c.bucket, c.num_rel) == []
    assert lists[3] == c.S * c.S // R.PAIR_SEG + c.num_rel
    if name == "one_each":
        assert int(lists[2][c.num_rel]) == lists[3] == 16      # the bound is met with equality: no empty segment behind the real ones
    if name == "synthetic":
        counts = torch.bincount(c.bucket.reshape(-1).long(), minlength=c.num_rel).tolist()
        assert counts[:len(R.SYNTH_COUNTS)] == list(R.SYNTH_COUNTS)
    if name == "joint":
        assert int(torch.bincount(c.bucket.reshape(-1).long()).max()) == 32896


def test_pair_list_checker_rejects_broken_lists():
    c = R.bucket_case("synthetic")
    pos, seg, bs, nseg = lists_of(c)
    assert R.check_pairs((pos, seg, bs, nseg), c.bucket, c.num_rel) == []
    p = pos.clone(); p[5] = p[6]
    assert R.check_pairs((p, seg, bs, nseg), c.bucket, c.num_rel)
    p = pos.clone(); p[[100, 101]] = p[[101, 100]]      # two positions of the largest bucket out of order
    assert R.check_pairs((p, seg, bs, nseg), c.bucket, c.num_rel)
    s = seg.clone(); s[2] += 1      # across a bucket edge
    assert R.check_pairs((pos, s, bs, nseg), c.bucket, c.num_rel)
    s = seg.clone(); s[-2] = 0
    assert R.check_pairs((pos, s, bs, nseg), c.bucket, c.num_rel)
    b = bs.clone(); b[3] += 1
    assert R.check_pairs((pos, seg, b, nseg), c.bucket, c.num_rel)
    assert R.check_pairs((pos, seg[:-1], bs, nseg), c.bucket, c.num_rel)


def test_pair_list_cache():
    hip = hipmod()
    tab = R.bucket_case("token257c").bucket.clone()
    a = hip.relpos_pairs(tab, 257, 514)
    assert hip.relpos_pairs(tab, 257, 514) is a                      # the same tensor, S and num_rel: the cached object
    b = hip.relpos_pairs(tab, 70, 514)                               # another S on the same tensor rebuilds
    assert b is not a and b[0].numel() == 70 * 70
    assert R.check_pairs(b, tab[:70, :70], 514) == []
    a2 = hip.relpos_pairs(tab, 257, 514)
    assert a2 is not b and all(torch.equal(x, y) for x, y in zip(a[:3], a2[:3]))
    tab[5, 7] = 3                                                    # an in-place write (version bump) rebuilds the lists
    a3 = hip.relpos_pairs(tab, 257, 514)
    assert a3 is not a2 and not torch.equal(a3[0], a2[0])
    assert R.check_pairs(a3, tab, 514) == []
    v1, v2 = tab[:33, :33], tab[:33, :33]                            # a fresh view does not reuse another view's lists
    l1 = hip.relpos_pairs(v1, 33, 514)
    l2 = hip.relpos_pairs(v2, 33, 514)
    assert l1 is not l2 and hip.relpos_pairs(v1, 33, 514) is l1
    assert all(torch.equal(x, y) for x, y in zip(l1[:3], l2[:3]))


def test_references_against_the_oracle():
    c = R.bucket_case("image4")
    heads, B, K = 3, 4, 9
    table = R.make_table(c.num_rel, heads).float().clamp(-8, 8)      # (finite sums for autograd)
    dense = O.rel_pos_bias(table, c.bucket.long())
    assert torch.equal(R.image_ref(table, c.bucket, 24)[:, :, :c.S], dense)
    assert torch.equal(R.image_ref(table, c.bucket, 24, True)[:, :, :c.S], dense.transpose(1, 2))
    assert float(R.image_ref(table, c.bucket, 24)[:, :, c.S:].abs().max()) == 0
    ids = R.make_ids("mixed", B, K, c.S)
    il = ids.long()
    full = dense.unsqueeze(0).expand(B, -1, -1, -1)
    want = torch.gather(torch.gather(full, 2, il[:, None, :, None].expand(-1, heads, -1, c.S)), 3, il[:, None, None, :].expand(-1, heads, K, -1))
    assert torch.equal(R.image_ids_ref(table, c.bucket, ids, 16)[..., :K], want)
    assert torch.equal(R.image_ids_ref(table, c.bucket, ids, 16, True)[..., :K], want.transpose(2, 3))
    # gradients through autograd in fp64
    t = table.double().requires_grad_()
    g = R.make_grad("real", (heads, c.S, 24), c.S, 1)
    O.rel_pos_bias(t, c.bucket.long()).backward(g[:, :, :c.S].double())
    ref, absum, counts = R.dtable_ref(g, c.bucket, c.num_rel)
    assert float((ref - t.grad).abs().max()) <= 1e-12 and int(counts.sum()) == c.S * c.S and bool((absum >= ref.abs() - 1e-12).all())
    t.grad = None
    gi = R.make_grad("real", (B, heads, K, 16), K, 2)
    d = O.rel_pos_bias(t, c.bucket.long()).unsqueeze(0).expand(B, -1, -1, -1)
    torch.gather(torch.gather(d, 2, il[:, None, :, None].expand(-1, heads, -1, c.S)), 3, il[:, None, None, :].expand(-1, heads, K, -1)).backward(gi[..., :K].double())
    dense64, _, cnt = R.fold_ref(gi, ids, c.S)
    assert int(cnt.sum()) == B * K * K
    assert float((R.dtable_ref(dense64, c.bucket, c.num_rel)[0] - t.grad).abs().max()) <= 1e-12


def test_id_sets():
    for kind in R.ID_KINDS:
        ids = R.make_ids(kind, 5, 9, 17)
        assert ids.dtype == I32 and ids.shape == (5, 9)
    s = R.make_ids("sorted", 5, 9, 17)
    assert bool((s[:, 0] == 0).all()) and bool((s.diff(dim=1) > 0).all())
    assert not bool((R.make_ids("unsorted", 5, 9, 17).diff(dim=1) > 0).all())
    assert any(r.unique().numel() < 9 for r in R.make_ids("repeats", 5, 9, 17))
    assert torch.equal(R.make_ids("mixed", 5, 9, 17)[3], torch.arange(9, dtype=I32))
    z = R.make_ids("shared0", 5, 9, 17)
    assert bool((z[:, 0] == 0).all()) and bool(((z == 0).sum(1) == 3).all())
    assert int(R.fold_ref(torch.zeros(5, 1, 9, 16), z, 17)[2][0, 0]) == 9 * 5


SHARES = {}


@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("name", R.BUCKET_NAMES)
def test_emulation_against_fp64(name, heads):
    c = R.bucket_case(name)
    lists = lists_of(c)
    for Spad in (c.S, R.attn_spad(c.S)):
        gi = R.make_grad("int", (heads, c.S, Spad), c.S, 3)
        ref, absum, counts = R.dtable_ref(gi, c.bucket, c.num_rel)
        assert float(absum.max()) < 2 ** 24
        assert torch.equal(R.emulate_bwd(gi, c.S, Spad, lists, c.num_rel).double(), ref), "int family, Spad %d" % Spad
        gr = R.make_grad("real", (heads, c.S, Spad), c.S, 4)
        ref, absum, counts = R.dtable_ref(gr, c.bucket, c.num_rel)
        got = R.emulate_bwd(gr, c.S, Spad, lists, c.num_rel)
        s, off = R.share(got, ref, R.bwd_budget(absum, counts))
        SHARES[name] = max(SHARES.get(name, 0.0), s)
        print("%s heads %d Spad %d: largest |err| / E_r = %.4f" % (name, heads, Spad, s))
        assert s <= 1 and off == 0      # (E_r == 0: an empty bucket, exactly 0)
        assert bool((got[counts == 0] == 0).all())
    print("largest share of E_r so far: %.4f (%s)" % (max(SHARES.values()), max(SHARES, key=SHARES.get)))


@pytest.mark.parametrize("mutant", R.BWD_MUTANTS)
@pytest.mark.parametrize("name", R.MUTANT_CASES)
def test_gates_reject_mutants(name, mutant):
    """Both sharp gates on each mutant: `int` equality with fp64, and the bits of the right re-statement on `real` data."""
    c = R.bucket_case(name)
    lists = lists_of(c)
    heads, Spad = 3, R.attn_spad(c.S)
    gi = R.make_grad("int", (heads, c.S, Spad), c.S, 5)
    ref = R.dtable_ref(gi, c.bucket, c.num_rel)[0]
    assert torch.equal(R.emulate_bwd(gi, c.S, Spad, lists, c.num_rel).double(), ref)
    bad = R.emulate_bwd(gi, c.S, Spad, lists, c.num_rel, mutant).double()
    assert not torch.equal(torch.nan_to_num(bad, nan=1e30), ref), "the int-equality gate lets %s pass" % mutant
    gr = R.make_grad("real", (heads, c.S, Spad), c.S, 6)
    good = R.emulate_bwd(gr, c.S, Spad, lists, c.num_rel)
    bad = R.emulate_bwd(gr, c.S, Spad, lists, c.num_rel, mutant)
    assert not torch.equal(good.view(I32), bad.view(I32)), "the bit comparison lets %s pass" % mutant


# ---- relpos.joint_handle's assembly, nothing launched -----------------------------------------------------------------------
class _Stub:
    def __init__(self, table, bucket_i32, S, ids=None):
        self.table, self.bucket, self.S, self.ids = table, bucket_i32, S, ids

    def dense(self, B):
        """What the handle's images must hold, [B, heads, K, K] fp32 (shared image: expanded)."""
        d = self.table.float()[self.bucket.long()].permute(2, 0, 1).unsqueeze(0).expand(B, -1, -1, -1)
        if self.ids is None:
            return d
        i = self.ids.long()
        return torch.stack([d[b][:, i[b]][:, :, i[b]] for b in range(B)])


def _specs():
    from one_peace_amd import relpos
    heads = 3
    ib = relpos.make_image_bucket_position(4, 52)
    tb = relpos.add_cls_buckets(relpos.make_token_bucket_position(8, 64), 15)[:24, :24]
    ab = relpos.add_cls_buckets(relpos.make_token_bucket_position(16, 64), 31)[:10, :10]
    g = torch.Generator().manual_seed(9)
    mk = lambda n, b: relpos.RelPosSpec(torch.randn(n, heads, generator=g), b)      # noqa: E731
    return relpos, mk(52, ib), mk(18, tb), mk(34, ab)


def test_joint_handle_assembly(monkeypatch):
    relpos, img, txt, aud = _specs()
    monkeypatch.setattr(relpos.ops, "RelPosBias", _Stub)
    B = 3
    # without ids: image + text
    cache = {}
    h = relpos.joint_handle([img, txt], [17, 24], cache)
    assert h.ids is None and h.S == 41 and h.bucket.dtype == I32 and tuple(h.bucket.shape) == (41, 41)
    assert tuple(h.table.shape) == (52 + 18 + 1, 3) and float(h.table[-1].abs().max()) == 0      # rows stacked, then the zero row
    assert torch.equal(h.table[:52], img.table) and torch.equal(h.table[52:70], txt.table)
    assert torch.equal(h.bucket[:17, :17], img.bucket.to(I32)) and torch.equal(h.bucket[17:, 17:], txt.bucket.to(I32) + 52)      # row bases
    assert bool((h.bucket[:17, 17:] == 70).all()) and bool((h.bucket[17:, :17] == 70).all())      # off the diagonal: the zero row
    d = h.dense(B)
    assert torch.equal(d[..., :17, :17], img.dense(B)) and torch.equal(d[..., 17:, 17:], txt.dense(B))
    assert float(d[..., :17, 17:].abs().max()) == 0 and float(d[..., 17:, :17].abs().max()) == 0
    h2 = relpos.joint_handle([img, txt], [17, 24], cache)      # the bucket cache: the same tensor for the same key
    assert h2.bucket is h.bucket and len(cache) == 1
    assert relpos.joint_handle([img, txt], [17, 24]).bucket is not h.bucket
    # three segments, the middle one without a bias: its block is the zero row too, and later row bases skip nothing
    h = relpos.joint_handle([img, None, aud], [17, 5, 10], cache)
    assert len(cache) == 2 and h.S == 32 and tuple(h.table.shape) == (52 + 34 + 1, 3)
    d = h.dense(B)
    assert torch.equal(d[..., :17, :17], img.dense(B)) and torch.equal(d[..., 22:, 22:], aud.dense(B))
    blk = torch.zeros(32, 32, dtype=torch.bool)
    blk[:17, :17] = blk[22:, 22:] = True
    assert float(d[..., ~blk].abs().max()) == 0 and bool((h.bucket[~blk] == 86).all())
    # ids on the image segment: the bucket covers the FULL positions, ids are offset by the segments' full lengths
    K = 6
    ids = R.make_ids("mixed", B, K, 17).long()
    im = img.with_ids(ids)
    h = relpos.joint_handle([im, txt], [K, 24], cache)
    assert tuple(h.bucket.shape) == (41, 41) and h.S == K + 24 and h.ids.dtype == I32 and tuple(h.ids.shape) == (B, K + 24)
    assert torch.equal(h.ids[:, :K], ids.to(I32)) and torch.equal(h.ids[:, K:], torch.arange(17, 41, dtype=I32).expand(B, -1))
    d = h.dense(B)
    assert torch.equal(d[..., :K, :K], im.dense(B)) and torch.equal(d[..., K:, K:], txt.dense(B))
    assert float(d[..., :K, K:].abs().max()) == 0 and float(d[..., K:, :K].abs().max()) == 0
    # ids on two segments with a None segment between them: arange over the None segment's own length
    tids = R.make_ids("sorted", B, 7, 24, seed=1).long()
    tx = txt.with_ids(tids)
    h = relpos.joint_handle([im, None, tx], [K, 4, 7], cache)
    assert tuple(h.bucket.shape) == (17 + 4 + 24,) * 2 and h.S == K + 4 + 7
    assert torch.equal(h.ids[:, :K], ids.to(I32)) and torch.equal(h.ids[:, K:K + 4], torch.arange(17, 21, dtype=I32).expand(B, -1))
    assert torch.equal(h.ids[:, K + 4:], tids.to(I32) + 21)
    d = h.dense(B)
    assert torch.equal(d[..., :K, :K], im.dense(B)) and torch.equal(d[..., K + 4:, K + 4:], tx.dense(B))
    blk = torch.zeros(K + 11, K + 11, dtype=torch.bool)
    blk[:K, :K] = blk[K + 4:, K + 4:] = True
    assert float(d[..., ~blk].abs().max()) == 0
    h2 = relpos.joint_handle([im, None, tx], [K, 4, 7], cache)
    assert h2.bucket is h.bucket and torch.equal(h2.ids, h.ids)
