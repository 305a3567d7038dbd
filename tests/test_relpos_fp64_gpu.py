"""The relative-position bias path on the device against exact references (tests/relpos_ref.py, checked on the CPU by
tests/test_relpos_ref_cpu.py): op_relpos_bias_build, op_relpos_bias_build_ids, op_relpos_bias_fold_ids and op_relpos_bias_bwd through the
C ABI, the pair lists of hip.relpos_pairs on device tensors, the autograd glue of ops.RelPosBias and relpos.joint_handle.

Every launch gets the caller's buffers: every output and every input lives in a guarded buffer (a sentinel bit pattern around it, checked
after the launches), inputs are compared bit for bit with their host copies afterwards, and outputs, partial_ws and dtable start as the
NaN sentinel.  The pad columns of every gradient hold NaN: a kernel that reads one shows it.

Gates: the images are compared bit for bit (pad columns +0).  Gradients of the `int` family must EQUAL the fp64 sum; those of the `real`
family must carry the bits of the host re-statement of op_relpos_bias_bwd (fixed order, additions only), stay inside the derived E_r, and
come out the same from a second launch and from rebuilt lists.  The fold adds with atomics: addresses with one contribution are
bit-exact, untouched ones +0, the others inside gamma(c - 1) sum|x| (at c = 2 that is ONE rounding of x1 + x2: among 10^5 addresses a
same-sign pair comes within 10^-4 of it, so the report shows a share of 1.0000 there).

Each case appends one line to relpos_fp64_report.txt in the tests' output directory: its id, the route (kernels, trips of each
grid-stride loop: more than one = past the grid cap) and for `real` data the largest share |err| / E.  relpos_seg_fold_kernel cannot
pass the grid cap at any configuration (tests/relpos_ref.py)."""
import gc
import os

import pytest
import torch

from tests import relpos_ref as R
from tests.gemm_ref import SENTINEL
from tests.util import out_dir

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32, I32 = R.BF, R.F32, R.I32
_INT = {BF: torch.int16, F32: torch.int32, I32: torch.int32}


def hipmod():
    from one_peace_amd import hip
    return hip


def bits(t):
    return t.contiguous().view(_INT[t.dtype])


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


class Run:
    """The guarded device tensors of one case, its failures and its largest shares."""
    reported = False      # the first case of a session starts relpos_fp64_report.txt afresh: one line per case

    def __init__(self, cid):
        self.cid, self.routes, self.fails, self.sh = cid, [], [], {}
        self.inputs, self.outputs = [], []

    def inp(self, host, ld=None):
        """A guarded device copy of a host tensor (compared with it at the end).  ld: a 2-D operand with that leading dimension."""
        host = host.contiguous() if ld is None else host
        if ld is not None:
            v = R.guarded_ld(tuple(host.shape), host.dtype, ld, device=DEV)
            v.copy_(host.to(DEV))
            self.inputs.append((v, host))
            return v
        flat = R.guarded_from(host.reshape(-1), device=DEV)
        self.inputs.append((flat, host.reshape(-1)))
        return flat.view(host.shape)

    def out(self, shape, dtype, zero=False):
        """A guarded output holding the sentinel (zero=True: zeros, for dense_ws)."""
        n = 1
        for s in shape:
            n *= s
        flat = R.guarded((n,), dtype, device=DEV)
        if zero:
            flat.zero_()
        self.outputs.append(flat)
        return flat.view(shape)

    def route(self, text):
        if text not in self.routes:
            self.routes.append(text)

    def require(self, ok, msg):
        if not ok:
            self.fails.append(msg)

    def share(self, key, got, exact, E):
        s, off = R.share(got, exact, E)
        self.sh[key] = max(self.sh.get(key, 0.0), s)
        self.require(off == 0, "%s: %d elements with a zero budget differ" % (key, off))
        self.require(s <= 1, "%s: |err| / E = %.3f" % (key, s))

    def finish(self):
        torch.cuda.synchronize()
        for v in self.outputs + [v for v, _ in self.inputs]:
            n = R.check_guard(v)
            self.require(n == 0, "%d guard elements overwritten around a buffer of %d elements" % (n, v.numel()))
        for v, host in self.inputs:
            self.require(torch.equal(bits(v.cpu()), bits(host)), "an input of shape %s changed" % (tuple(v.shape),))
        line = "%s route %s shares %s" % (self.cid, "; ".join(self.routes), " ".join("%s=%.4f" % kv for kv in sorted(self.sh.items())) or "(exact)")
        with open(os.path.join(out_dir(), "relpos_fp64_report.txt"), "a" if Run.reported else "w") as f:
            f.write(line + "\n")
        Run.reported = True
        print(line)
        assert not self.fails, "\n".join(self.fails[:12])


def sentinel_left(t):
    return int((bits(t) == SENTINEL[t.dtype][1]).sum())


# ---- launches through the C ABI --------------------------------------------------------------------------------------------
def rc_build(table, bucket, ld, out, heads, S, Spad, transposed):
    hip = hipmod()
    return hip.lib().op_relpos_bias_build(hip.ptr(table), hip.ptr(bucket), ld, hip.ptr(out), heads, S, Spad, int(transposed), hip.stream())


def rc_build_ids(table, bucket, ld, ids, out, B, heads, K, Kpad, transposed):
    hip = hipmod()
    return hip.lib().op_relpos_bias_build_ids(hip.ptr(table), hip.ptr(bucket), ld, hip.ptr(ids), hip.ptr(out), B, heads, K, Kpad, int(transposed),
                                              hip.stream())


def rc_fold(dbias, ids, dense, Sfull, B, heads, K, Kpad):
    hip = hipmod()
    return hip.lib().op_relpos_bias_fold_ids(hip.ptr(dbias), hip.ptr(ids), hip.ptr(dense), Sfull, B, heads, K, Kpad, hip.stream())


def rc_bwd(dbias, S, Spad, pos, seg, nseg, bucket_seg, num_rel, partial, dtable, heads):
    hip = hipmod()
    return hip.lib().op_relpos_bias_bwd(hip.ptr(dbias), S, Spad, hip.ptr(pos), hip.ptr(seg), nseg, hip.ptr(bucket_seg), num_rel, hip.ptr(partial),
                                        hip.ptr(dtable), heads, hip.stream())


def ok(rc, what):
    hipmod()._check(rc, what)


_DEVICE = {}


def dev_bucket(name):
    """(case, an UNGUARDED contiguous device copy of its bucket for hip.relpos_pairs, the CPU lists of the same bucket)."""
    if name not in _DEVICE:
        hip = hipmod()
        c = R.bucket_case(name)
        _DEVICE[name] = (c, c.bucket.contiguous().to(DEV), hip.relpos_pairs(c.bucket.contiguous().clone(), c.S, c.num_rel))
    return _DEVICE[name]


def bucket_input(run, c, ld):
    """The case's bucket as a guarded launch operand of leading dimension ld."""
    return run.inp(c.bucket, ld=ld)


def lds_of(c):
    """bucket_ld values of a case: S and, where the bucket fits a 1024-wide table, 1024 (an uncopied [:S, :S] view)."""
    return (c.S, 1024) if c.S <= 1024 else (c.S,)


def bwd_launch(run, dbias_dev, S, Spad, lists, num_rel, heads):
    pos, seg, bs, nseg = lists
    partial = run.out((nseg, heads), F32)
    dtable = run.out((num_rel, heads), F32)
    ok(rc_bwd(dbias_dev, S, Spad, pos, seg, nseg, bs, num_rel, partial, dtable, heads), "op_relpos_bias_bwd")
    run.route("seg_sum trips=%d, seg_fold trips=%d" % (R.trips(nseg * heads), R.trips(num_rel * heads)))
    return dtable, partial


# ---- op_relpos_bias_build -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.BUCKET_NAMES)
def test_build(name):
    c = R.bucket_case(name)
    run = Run("build-%s" % name)
    for heads in R.HEADS + ((2,) if name == "image32" else ()):      # (n = 32, heads = 2: the issue's grid-stride case, S Spad > 2048 x 256)
        table_h = R.make_table(c.num_rel, heads)
        table = run.inp(table_h)
        tdev = table_h.to(DEV)
        for ld in ((c.ld,) if name.startswith("token") else lds_of(c)):
            bucket = bucket_input(run, c, ld)
            for Spad in R.spads(c.S):
                for tr in (False, True):
                    out = run.out((heads, c.S, Spad), BF)
                    ok(rc_build(table, bucket, ld, out, heads, c.S, Spad, tr), "op_relpos_bias_build")
                    run.require(same(out, R.image_ref(tdev, bucket, Spad, tr)), "heads %d ld %d Spad %d transposed %d: the image differs" % (heads, ld, Spad, tr))
                    run.route("build ld=%s trips=%d" % ("S" if ld == c.S else ld, R.trips(c.S * Spad)))
    run.finish()


# ---- op_relpos_bias_build_ids / op_relpos_bias_fold_ids -------------------------------------------------------------------
IDS_PARAMS = [(i, kind) for i, case in enumerate(R.IDS_CASES) for kind in case[5]]


def ids_id(p):
    B, K, Kpad, name, heads, _ = R.IDS_CASES[p[0]]
    return "B%d-K%d-Kpad%d-%s-h%d-%s" % (B, K, Kpad, name, heads, p[1])


@pytest.mark.parametrize("p", IDS_PARAMS, ids=ids_id)
def test_build_ids(p):
    B, K, Kpad, name, heads, _ = R.IDS_CASES[p[0]]
    kind = p[1]
    c = R.bucket_case(name)
    run = Run("build_ids-" + ids_id(p))
    ld = 1024 if (c.S <= 1024 and R.ID_KINDS.index(kind) % 2) else c.S
    table_h = R.make_table(c.num_rel, heads)
    table, bucket = run.inp(table_h), bucket_input(run, c, ld)
    ids = run.inp(R.make_ids(kind, B, K, c.S, seed=p[0]))
    for tr in (False, True):
        out = run.out((B, heads, K, Kpad), BF)
        ok(rc_build_ids(table, bucket, ld, ids, out, B, heads, K, Kpad, tr), "op_relpos_bias_build_ids")
        run.require(same(out, R.image_ids_ref(table_h.to(DEV), bucket, ids, Kpad, tr)), "transposed %d: the images differ" % tr)
    run.route("build_ids ld=%s trips=%d" % ("S" if ld == c.S else ld, R.trips(B * K * Kpad)))
    run.finish()


@pytest.mark.parametrize("family", ["int", "real"])
@pytest.mark.parametrize("p", IDS_PARAMS, ids=ids_id)
def test_fold_ids(p, family):
    """The fold on a zeroed dense_ws; `int`: then op_relpos_bias_bwd over the folded image (S = Spad = Sfull), exact end to end."""
    B, K, Kpad, name, heads, _ = R.IDS_CASES[p[0]]
    c, bdev, _ = dev_bucket(name)
    S = c.S
    run = Run("fold_ids-%s-%s" % (ids_id(p), family))
    g_h = R.make_grad(family, (B, heads, K, Kpad), K, 10 + p[0])
    ids_h = R.make_ids(p[1], B, K, S, seed=p[0])
    g, ids = run.inp(g_h), run.inp(ids_h)
    dense = run.out((heads, S, S), F32, zero=True)
    ok(rc_fold(g, ids, dense, S, B, heads, K, Kpad), "op_relpos_bias_fold_ids")
    run.route("fold_ids trips=%d, most adds on one address %d" % (R.trips(B * heads * K * K), int(R.fold_ref(g_h[:, :1], ids_h, S)[2].max())))
    ref, absum, count = R.fold_ref(g, ids, S)
    if p[1] == "shared0":
        run.require(int(count[0, 0]) == 9 * B, "the shared position has %d contributions" % int(count[0, 0]))
    run.require(not bool(torch.isnan(dense).any()), "NaN in dense_ws: a pad column was read")
    run.require(int(bits(dense)[:, count == 0].ne(0).sum()) == 0, "an address without a contribution is not +0")
    if family == "int":
        run.require(torch.equal(dense.double(), ref), "int family: dense_ws differs from the fp64 scatter")
        hip = hipmod()
        dtable, _ = bwd_launch(run, dense, S, S, hip.relpos_pairs(bdev, S, c.num_rel), c.num_rel, heads)
        want, absum_t, _ = R.dtable_ref(ref, bdev, c.num_rel)
        run.require(float(absum_t.max()) < 2 ** 24, "the case leaves the range in which fp32 is exact")
        run.require(torch.equal(dtable.double(), want), "int family: fold + table gradient differs from fp64")
    else:
        one = (count == 1)[None].expand_as(ref)
        run.require(torch.equal(dense.double()[one], ref[one]), "an address with one contribution is not bit-exact")
        run.share("fold", dense, ref, R.fold_budget(absum, count))
    run.finish()


# ---- op_relpos_bias_bwd ---------------------------------------------------------------------------------------------------
def bwd_params():
    out = []
    for name in R.BUCKET_NAMES:
        S = R.bucket_case(name).S
        for heads in R.HEADS + ((16,) if name == "image32" else ()):      # (n = 32, heads = 16: nseg heads = 588 864 > 2048 x 256)
            for Spad in sorted({S, R.attn_spad(S)}):
                out.append((name, heads, Spad))
    return out


@pytest.mark.parametrize("name,heads,Spad", bwd_params())
def test_bwd(name, heads, Spad):
    hip = hipmod()
    c, bdev, cpu_lists = dev_bucket(name)
    S = c.S
    run = Run("bwd-%s-h%d-Spad%d" % (name, heads, Spad))
    if name.startswith("token") and name.endswith("v"):      # the uncopied view: the lists are built from a [:S, :S] view of a 1024-wide device table
        full = torch.zeros(1024, 1024, dtype=I32, device=DEV)
        full[:S, :S] = bdev
        lists = hip.relpos_pairs(full[:S, :S], S, c.num_rel)
    else:
        lists = hip.relpos_pairs(bdev, S, c.num_rel)
    run.require(lists[3] == cpu_lists[3] and all(torch.equal(a.cpu(), b) for a, b in zip(lists[:3], cpu_lists[:3])), "the device lists differ from the CPU lists")
    run.require(all(t.dtype == I32 and t.is_contiguous() for t in lists[:3]), "the lists are not contiguous int32")
    counts = torch.bincount(bdev.reshape(-1).long(), minlength=c.num_rel)
    for family in ("int", "real"):
        g_h = R.make_grad(family, (heads, S, Spad), S, 20)
        g = run.inp(g_h)
        dtable, partial = bwd_launch(run, g, S, Spad, lists, c.num_rel, heads)
        ref, absum, _ = R.dtable_ref(g, bdev, c.num_rel)
        run.require(sentinel_left(dtable) == 0, "%s: dtable keeps its sentinel somewhere: not overwritten" % family)
        run.require(not bool(torch.isnan(dtable).any()) and not bool(torch.isnan(partial).any()), "%s: NaN (a pad column or an unwritten workspace slot was read)" % family)
        run.require(int(bits(dtable)[counts == 0].ne(0).sum()) == 0, "%s: an empty bucket is not +0" % family)
        if family == "int":
            run.require(float(absum.max()) < 2 ** 24, "the case leaves the range in which fp32 is exact")
            run.require(torch.equal(dtable.double(), ref), "int family: dtable differs from the fp64 sum")
        else:
            emu = R.emulate_bwd(g_h, S, Spad, cpu_lists, c.num_rel)
            run.require(same(dtable.cpu(), emu), "real family: dtable has not the bits of the host re-statement (%d of %d elements differ)"
                        % (int((bits(dtable.cpu()) != bits(emu)).sum()), emu.numel()))
            run.share("dtable", dtable, ref, R.bwd_budget(absum, counts))
            again, _ = bwd_launch(run, g, S, Spad, lists, c.num_rel, heads)
            run.require(same(again, dtable), "a second launch gives other bits")
            rebuilt, _ = bwd_launch(run, g, S, Spad, hip.relpos_pairs(bdev.clone(), S, c.num_rel), c.num_rel, heads)
            run.require(same(rebuilt, dtable), "rebuilt lists give other bits")
    run.finish()


# ---- the wrappers return the bits of the C-ABI launch ---------------------------------------------------------------------
def test_wrappers():
    hip = hipmod()
    c, bdev, _ = dev_bucket("image16")
    S, heads, Spad = c.S, 3, R.attn_spad(c.S)
    run = Run("wrappers")
    table = R.make_table(c.num_rel, heads).to(DEV)
    for tr in (False, True):
        out = run.out((heads, S, Spad), BF)
        ok(rc_build(table, bdev, S, out, heads, S, Spad, tr), "op_relpos_bias_build")
        run.require(same(hip.relpos_bias_build(table, bdev, S, Spad, transposed=tr), out), "relpos_bias_build, transposed %d" % tr)
    view = torch.zeros(1024, 1024, dtype=I32, device=DEV)
    view[:S, :S] = bdev
    run.require(same(hip.relpos_bias_build(table, view[:S, :S], S, Spad), R.image_ref(table, bdev, Spad)), "relpos_bias_build on a view")
    B, K, Kpad = 4, 120, 128
    ids = R.make_ids("mixed", B, K, S).to(DEV)
    for tr in (False, True):
        out = run.out((B, heads, K, Kpad), BF)
        ok(rc_build_ids(table, bdev, S, ids, out, B, heads, K, Kpad, tr), "op_relpos_bias_build_ids")
        run.require(same(hip.relpos_bias_build_ids(table, bdev, ids, Kpad, transposed=tr), out), "relpos_bias_build_ids, transposed %d" % tr)
    g = R.make_grad("real", (heads, S, Spad), S, 30).to(DEV)
    dtable, _ = bwd_launch(run, g, S, Spad, hip.relpos_pairs(bdev, S, c.num_rel), c.num_rel, heads)
    run.require(same(hip.relpos_bias_bwd(g, bdev, c.num_rel, S, Spad), dtable), "relpos_bias_bwd")
    gi = R.make_grad("int", (B, heads, K, Kpad), K, 31).to(DEV)      # (`int`: the fold's atomics add in no fixed order)
    dense = run.out((heads, S, S), F32, zero=True)
    ok(rc_fold(gi, ids, dense, S, B, heads, K, Kpad), "op_relpos_bias_fold_ids")
    dtable, _ = bwd_launch(run, dense, S, S, hip.relpos_pairs(bdev, S, c.num_rel), c.num_rel, heads)
    run.require(same(hip.relpos_bias_bwd_ids(gi, bdev, ids, c.num_rel), dtable), "relpos_bias_bwd_ids")
    run.route("wrappers of build, build_ids, bwd, bwd_ids")
    run.finish()


# ---- refusals: nothing is launched, the outputs keep their sentinel ---------------------------------------------------------
def test_refusals():
    c, bdev, _ = dev_bucket("image4")
    hip = hipmod()
    S, heads, Spad, B, K, Kpad = c.S, 3, 24, 2, 9, 16
    run = Run("refusals")
    table = R.make_table(c.num_rel, heads).to(DEV)
    ids = R.make_ids("sorted", B, K, S).to(DEV)
    pos, seg, bs, nseg = hip.relpos_pairs(bdev, S, c.num_rel)
    img, imgs = run.out((heads, S, Spad), BF), run.out((B, heads, K, Kpad), BF)
    dense, partial, dtable = run.out((heads, S, S), F32), run.out((nseg, heads), F32), run.out((c.num_rel, heads), F32)
    g, gi = torch.zeros(heads, S, Spad, device=DEV), torch.zeros(B, heads, K, Kpad, device=DEV)
    calls = {
        "build Spad < S": lambda: rc_build(table, bdev, S, img, heads, S, 16, 0),
        "build Spad % 8": lambda: rc_build(table, bdev, S, img, heads, S, 20, 0),
        "build null table": lambda: rc_build(None, bdev, S, img, heads, S, Spad, 0),
        "build null bucket": lambda: rc_build(table, None, S, img, heads, S, Spad, 0),
        "build null out": lambda: rc_build(table, bdev, S, None, heads, S, Spad, 0),
        "build_ids B = 0": lambda: rc_build_ids(table, bdev, S, ids, imgs, 0, heads, K, Kpad, 0),
        "build_ids K = 0": lambda: rc_build_ids(table, bdev, S, ids, imgs, B, heads, 0, Kpad, 0),
        "build_ids Kpad < K": lambda: rc_build_ids(table, bdev, S, ids, imgs, B, heads, K, 8, 0),
        "build_ids Kpad % 8": lambda: rc_build_ids(table, bdev, S, ids, imgs, B, heads, K, 12, 0),
        "fold B = 0": lambda: rc_fold(gi, ids, dense, S, 0, heads, K, Kpad),
        "fold K = 0": lambda: rc_fold(gi, ids, dense, S, B, heads, 0, Kpad),
        "fold Sfull = 0": lambda: rc_fold(gi, ids, dense, 0, B, heads, K, Kpad),
        "bwd null pos": lambda: rc_bwd(g, S, Spad, None, seg, nseg, bs, c.num_rel, partial, dtable, heads),
        "bwd null seg": lambda: rc_bwd(g, S, Spad, pos, None, nseg, bs, c.num_rel, partial, dtable, heads),
        "bwd null bucket_seg": lambda: rc_bwd(g, S, Spad, pos, seg, nseg, None, c.num_rel, partial, dtable, heads),
        "bwd null dtable": lambda: rc_bwd(g, S, Spad, pos, seg, nseg, bs, c.num_rel, partial, None, heads),
        "bwd null partial_ws, nseg > 0": lambda: rc_bwd(g, S, Spad, pos, seg, nseg, bs, c.num_rel, None, dtable, heads),
        "bwd S = 0": lambda: rc_bwd(g, 0, Spad, pos, seg, nseg, bs, c.num_rel, partial, dtable, heads),
        "bwd Spad < S": lambda: rc_bwd(g, S, S - 1, pos, seg, nseg, bs, c.num_rel, partial, dtable, heads),
        "bwd num_rel = 0": lambda: rc_bwd(g, S, Spad, pos, seg, nseg, bs, 0, partial, dtable, heads),
        "bwd heads = 0": lambda: rc_bwd(g, S, Spad, pos, seg, nseg, bs, c.num_rel, partial, dtable, 0),
        "bwd nseg < 0": lambda: rc_bwd(g, S, Spad, pos, seg, -1, bs, c.num_rel, partial, dtable, heads),
        "bwd S = 46341 (S^2 >= 2^31)": lambda: rc_bwd(g, 46341, 46344, pos, seg, nseg, bs, c.num_rel, partial, dtable, heads),
    }
    for what, call in calls.items():
        rc = call()
        run.require(rc != 0, "%s is accepted" % what)
        if rc != 0:
            run.require(bool(hip.lib().op_last_error()), "%s: no error text" % what)
    torch.cuda.synchronize()
    for t in (img, imgs, dense, partial, dtable):
        run.require(sentinel_left(t) == t.numel(), "a refused call wrote to an output")
    run.route("%d refused calls, nothing launched" % len(calls))
    run.finish()


# ---- the autograd glue ----------------------------------------------------------------------------------------------------
def leaf_table(num_rel, heads):
    return R.make_table(num_rel, heads).to(DEV).requires_grad_()


def fill_acc(acc, live, seed):
    """`int` data in every slab of an accumulator; columns >= live hold NaN.  Returns the host copy."""
    g = R.make_grad("int", tuple(acc.shape), live, seed)
    acc.copy_(g.to(DEV))
    return g


def bf_of(x64):
    return x64.float().to(BF)      # (integers below 2^24: the step through fp32 is exact, ONE rounding to bf16)


@pytest.mark.parametrize("with_ids", [False, True])
def test_autograd_glue(with_ids):
    from one_peace_amd import ops
    c, bdev, _ = dev_bucket("image4")
    heads, B, K = 3, 5, 9
    run = Run("glue-%s" % ("ids" if with_ids else "shared"))
    table = leaf_table(c.num_rel, heads)
    ids = R.make_ids("mixed", B, K, c.S).to(DEV) if with_ids else None
    h = ops.RelPosBias(table, bdev, K if with_ids else c.S, ids=ids)
    Spad = R.attn_spad(h.S)
    if with_ids:
        want, wantT = (R.image_ids_ref(table.detach(), bdev, ids, Spad, tr) for tr in (False, True))
    else:
        want, wantT = (R.image_ref(table.detach(), bdev, Spad, tr) for tr in (False, True))
    run.require(same(h.image.detach(), want) and same(h.imageT, wantT), "image / imageT differ from the build kernels' images")
    acc = h.grad_accumulator(B)
    run.require(acc.dtype == F32 and tuple(acc.shape[1:]) == (heads, h.S, Spad) and (not with_ids or acc.shape[0] == B), "accumulator shape %s" % (tuple(acc.shape),))
    run.require(int(acc.ne(0).sum()) == 0, "a fresh accumulator is not zero")
    run.require(h.grad_accumulator(B) is acc, "the accumulator is not kept between layers")
    g = fill_acc(acc, h.S, 40)
    h.image.backward(torch.zeros_like(h.image))
    if with_ids:
        want = R.dtable_ref(R.fold_ref(g.to(DEV), ids, c.S)[0], bdev, c.num_rel)[0]
    else:
        want = R.dtable_ref(g[..., :h.S].double().sum(0).to(DEV), bdev, c.num_rel)[0]
    run.require(table.grad is not None and table.grad.dtype == BF and same(table.grad, bf_of(want)), "table.grad differs from the fp64 sum rounded once to bf16")
    run.require(h.acc is None, "the accumulator survives the backward")
    run.route("RelPosBias %s: %d slabs" % ("build_ids + fold_ids + bwd" if with_ids else "build + sum(0) + bwd", g.shape[0]))
    run.finish()


def test_slab_growth():
    """Layers that skip dropped samples ask for accumulators of different batch sizes: the grown one keeps what was added."""
    from one_peace_amd import hip, ops
    c, bdev, _ = dev_bucket("image4")
    heads = 3
    tune = hip.TUNE.attn_bwd()
    slabs = {B: hip.lib().op_attn_bwd_dbias_slabs(B, c.S, heads, tune) for B in range(1, 65)}
    B1 = next(B for B in slabs if slabs[B] >= 2)
    B2 = next(B for B in slabs if slabs[B] > slabs[B1])
    run = Run("glue-slab-growth")
    table = leaf_table(c.num_rel, heads)
    h = ops.RelPosBias(table, bdev, c.S)
    a1 = h.grad_accumulator(B1)
    assert a1.shape[0] == slabs[B1]
    g1 = fill_acc(a1, c.S, 41)
    keep = a1.clone()
    run.require(h.grad_accumulator(1) is a1, "a smaller batch replaced the accumulator")
    a2 = h.grad_accumulator(B2)
    assert a2.shape[0] == slabs[B2] > slabs[B1] and a2 is h.acc
    run.require(same(a2[:slabs[B1]], keep), "the grown accumulator lost the old slabs' bits")
    run.require(int(bits(a2[slabs[B1]:]).ne(0).sum()) == 0, "the new slabs are not zero")
    g2 = R.make_grad("int", tuple(a2.shape[1:]), c.S, 42)
    a2[-1].copy_(g2.to(DEV))      # a later layer adds into the last new slab
    h.image.backward(torch.zeros_like(h.image))
    want = R.dtable_ref((g1[..., :c.S].double().sum(0) + g2[..., :c.S].double()).to(DEV), bdev, c.num_rel)[0]
    run.require(same(table.grad, bf_of(want)), "the gradient does not count every slab")
    run.require(h.acc is None, "the accumulator survives the backward")
    run.route("grad_accumulator B %d -> %d: slabs %d -> %d" % (B1, B2, slabs[B1], slabs[B2]))
    run.finish()


@pytest.mark.parametrize("dropped", [True, False])
def test_backward_without_accumulator(dropped):
    """The handle dropped before the backward (or never asked for an accumulator): a zero bf16 gradient of the table's shape."""
    from one_peace_amd import ops
    c, bdev, _ = dev_bucket("image4")
    run = Run("glue-%s" % ("dead-handle" if dropped else "no-accumulator"))
    table = leaf_table(c.num_rel, 3)
    h = ops.RelPosBias(table, bdev, c.S)
    img = h.image
    if dropped:
        del h
        gc.collect()
    img.backward(torch.zeros_like(img))
    run.require(table.grad is not None and table.grad.dtype == BF and table.grad.shape == table.shape and int(bits(table.grad).ne(0).sum()) == 0,
                "no zero gradient of the table's shape")
    run.route("_RelPosImageFn.backward without an accumulator")
    run.finish()


# ---- relpos.joint_handle on the device ------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plain", "ids", "none-segment"])
def test_joint_handle(form):
    from one_peace_amd import relpos
    heads, B, K, T = 3, 4, 9, 24
    ci = R.bucket_case("image4")
    tb = R.bucket_case("token33c").bucket[:T, :T].long()
    num_t = R.bucket_case("token33c").num_rel
    run = Run("joint-%s" % form)
    ti, tt = leaf_table(ci.num_rel, heads), leaf_table(num_t, heads)
    img = relpos.RelPosSpec(ti, ci.bucket.long().to(DEV))
    txt = relpos.RelPosSpec(tt, tb.to(DEV))
    ids = R.make_ids("mixed", B, K, ci.S).long().to(DEV)
    if form == "plain":
        specs, lens, blocks = [img, txt], [ci.S, T], [(img, 0, ci.S, 0), (txt, ci.S, T, ci.S)]
    elif form == "ids":
        specs, lens, blocks = [img.with_ids(ids), txt], [K, T], [(img.with_ids(ids), 0, K, 0), (txt, K, T, ci.S)]
    else:
        specs, lens, blocks = [img.with_ids(ids), None, txt], [K, 5, T], [(img.with_ids(ids), 0, K, 0), (txt, K + 5, T, ci.S + 5)]
    # blocks: (spec, first token of the block in the stream, tokens, first FULL position of the block)
    cache = {}
    h = relpos.joint_handle(specs, lens, cache)
    S, Spad = sum(lens), R.attn_spad(sum(lens))
    per_sample = form != "plain"
    want = torch.zeros((B if per_sample else 1), heads, S, Spad, dtype=BF, device=DEV)
    for sp, o, n, _ in blocks:
        want[:, :, o:o + n, o:o + n] = sp.dense(B if per_sample else 1).detach().to(BF)
    got = h.image.detach() if per_sample else h.image.detach()[None]
    run.require(same(got, want), "the image is not the block-diagonal of the segments' dense()")
    wantT = torch.nn.functional.pad(want[..., :S].transpose(2, 3), (0, Spad - S))
    run.require(same(h.imageT if per_sample else h.imageT[None], wantT), "imageT is not its transpose")
    h2 = relpos.joint_handle(specs, lens, cache)
    run.require(len(cache) == 1 and h2.bucket is h.bucket and same(h2.image.detach(), h.image.detach()), "a second call does not reuse the cached bucket or gives other bits")
    del h2
    acc = h.grad_accumulator(B)
    g = fill_acc(acc, S, 50)
    h.image.backward(torch.zeros_like(h.image))
    g64 = g[..., :S].double().to(DEV)
    for sp, o, n, _ in blocks:
        blk = g64[:, :, o:o + n, o:o + n].contiguous()
        if sp.ids is not None:
            dense = R.fold_ref(blk, sp.ids.to(I32), sp.bucket.shape[0])[0]
        else:
            dense = blk.sum(0)
        want_t = R.dtable_ref(dense, sp.bucket.to(I32), sp.table.shape[0])[0]
        run.require(sp.table.grad is not None and same(sp.table.grad, bf_of(want_t)), "a modality's table does not receive exactly its block's sums (block at %d)" % o)
    run.require(h.acc is None, "the accumulator survives the backward")
    run.route("joint_handle %s: S %d, %d slabs" % (form, S, g.shape[0]))
    run.finish()
