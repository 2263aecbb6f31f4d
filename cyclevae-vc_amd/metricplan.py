"""The arena and the job tables of a device-side metric pass, built in one place (validation.ValidationPass.metrics,
stage5.CvgvPass.metrics, decode.DecodePass.metrics, trainlog.TrainLog._close).

A metric pass is: cvae_eval_stats (phase 1: reductions of the fp32 pass outputs, and their speech frames gathered into packed f64
matrices), cvae_dtw_batch (alignments of those matrices), cvae_eval_stats again (phase 2: figures of what the alignments wrote), and
one copy of the results to the host.  Everything the kernels write lives in ONE float64 arena, [results | scratch], and one int64
buffer (the alignments' twf rows).  A caller declares regions, jobs and alignments in any order; an operand is a device address (an
int, see row()) or a Ref, and Refs become addresses only in finalise(), when the sizes are known -- no caller adds offsets to
pointers.  The plan keeps every tensor whose address it gave to the device.
"""
import ctypes as C
import struct

import numpy as np
import torch

import _cabi
import gru_vae


def _packer(structure, names):
    """struct.Struct of a _cabi structure, from its _fields_: the tables are packed in one go, which costs a quarter of a ctypes
    object per job.  names: the field order finalise() packs in -- another order or layout in _cabi is an error here, at import."""
    code = {C.c_int32: "i", C.c_int64: "q", C.c_uint64: "Q", C.c_void_p: "Q"}
    fmt = "="
    for name, ctype in structure._fields_:
        assert struct.calcsize(fmt) == getattr(structure, name).offset, (structure.__name__, name)      # (no padding before it)
        fmt += code[ctype]
    assert tuple(n for n, _ in structure._fields_) == names and struct.calcsize(fmt) == C.sizeof(structure), structure.__name__
    return struct.Struct(fmt)


_JOB = _packer(_cabi.StatJob, ("kind", "rows", "c0", "c1", "src_rows", "pad_", "a", "b", "lda", "ldb", "idx", "dst", "out_off"))
_PROBLEM = _packer(_cabi.DtwProblem, ("org", "trg", "ld_org", "ld_trg", "T1", "T2", "D", "mcd", "aligned", "twf", "frames", "mean_out"))
RESULT, SCRATCH, OUTSIDE = 0, 1, 2      # Ref.seg: the two parts of the f64 arena; a device matrix outside it


def ints(v):
    return [int(x) for x in (v.tolist() if hasattr(v, "tolist") else v)]


def batch_rows(y, B):
    """y_in of one row or of B rows as a contiguous float32 [B, 1, C]"""
    y = y.to(torch.float32).reshape(-1, 1, y.shape[-1])
    return y[:1].expand(B, 1, y.shape[-1]).contiguous() if y.shape[0] != B else y


def row(t, j, col=0):
    """address of t[j, 0, col] of a contiguous [B, T, C] fp32 tensor, and its row stride"""
    return t.data_ptr() + 4 * (j * t.shape[1] * t.shape[2] + col), t.shape[2]


class Ref(object):
    """rows x cols float64 values at element `off` of a part of the arena (results: the offset in the host copy too); addr: their
    device address, known behind finalise()."""
    __slots__ = ("seg", "off", "rows", "cols", "addr")

    def __init__(self, seg, off, rows, cols, addr=None):
        self.seg, self.off, self.rows, self.cols, self.addr = seg, off, rows, cols, addr

    def of(self, host):
        """this result vector's values in the host copy (a scalar's value is host[off])"""
        return host[self.off:self.off + self.cols].copy()


class MetricPlan(object):
    """MetricPlan(dev, profile=False).  Declare: vec() (a result vector; one value by default), mat() (scratch), stat(), align(),
    latent_distance().  Then finalise() and the steps begin(), stats(1), dtw(), stats(2) on the current stream -- a caller may put
    launches of its own between them -- and results(), the device view to copy.  profile: events around the steps; times() after
    the copy."""

    def __init__(self, dev, profile=False):
        self.dev, self.n_out, self.n_scratch, self.n_twf = dev, 0, 0, 0      # n_out: the results, [0, n_out) of the arena
        self.jobs, self.probs, self.kept, self.refs, self.t1max, self.t2max = ([], []), [], [], [], 0, 0
        self.arena = self.twf = self.jdev = self.work = self.work_bytes = None
        # (profiling: the events exist before the first is recorded -- making one between a launch and its mark would count as the step's)
        self._ev, self._spare = ([], [torch.cuda.Event(enable_timing=True) for _ in range(12)]) if profile else (None, None)

    # ---- layout ------------------------------------------------------------------------------------------------------------------
    def vec(self, n=1):
        r = Ref(RESULT, self.n_out, 1, n)
        self.n_out += n
        self.refs.append(r)
        return r

    def mat(self, rows, cols):
        r = Ref(SCRATCH, self.n_scratch, rows, cols)
        self.n_scratch += rows * cols
        self.refs.append(r)
        return r

    def hold(self, t):
        self.kept.append(t)
        return t

    def f64(self, t):
        """a contiguous float64 device matrix as an operand of align()"""
        return Ref(OUTSIDE, 0, t.shape[0], t.shape[1], self.hold(t).data_ptr())

    # ---- jobs --------------------------------------------------------------------------------------------------------------------
    def stat(self, phase, kind, rows, c0, c1, a, lda, b=None, ldb=0, idx=None, dst=None, out=None, src_rows=0):
        """One reduction of cvae_eval_stats in phase 1 or 2: a, b, dst are addresses or Refs, out the result region it writes."""
        self.jobs[phase - 1].append((kind, rows, c0, c1, src_rows, a, b, lda, ldb, idx, dst, 0 if out is None else out.off))

    def align(self, org, trg, mcd, aligned=None, mean=None, c0=0):
        """One alignment of org to trg (Refs) over the columns from c0 on; aligned: a mat of trg's shape that receives the aligned
        sequence, mean: where the mean cost goes (nobody reads it when None).  Returns the region of the T2 frame costs."""
        T1, T2 = org.rows, trg.rows
        frames = self.mat(1, T2)
        if mean is None:
            self.n_scratch += 1      # (an unread mean goes behind the frame costs)
        if T1 > self.t1max:
            self.t1max = T1
        if T2 > self.t2max:
            self.t2max = T2
        self.probs.append((org, trg, c0, mcd, aligned, self.n_twf, frames, mean))
        self.n_twf += T2      # (the problem's twf row in the int64 buffer)
        return frames

    def latent_distance(self, gs, gt):
        """The script's latent distance of two packed sequences: a mel-cd alignment that writes the aligned sequence and a cosine
        alignment whose mean cost is the figure, in both directions, and the distance of each aligned sequence to what it was aligned
        to.  Returns the result scalars (rmse_a, rmse_b, cos_a, cos_b): the two figures are (a + b) / 2 each."""
        rmse_a, rmse_b, cos_a, cos_b = self.vec(), self.vec(), self.vec(), self.vec()
        for org, trg, rmse, cos in ((gs, gt, rmse_a, cos_a), (gt, gs, rmse_b, cos_b)):
            al = self.mat(trg.rows, trg.cols)
            self.align(org, trg, -1, al)
            self.align(trg, org, 0, None, cos)
            self.stat(2, _cabi.STAT_LATDIST, trg.rows, 0, trg.cols, al, trg.cols, trg, trg.cols, out=rmse)
        return rmse_a, rmse_b, cos_a, cos_b

    # ---- execution ---------------------------------------------------------------------------------------------------------------
    def resolve(self, fields):
        """a job's fields with the Refs among them as addresses (behind finalise())"""
        return [x.addr if x.__class__ is Ref else x for x in fields]

    def view(self, r):
        """a scratch region as a [rows, cols] view of the arena"""
        at = self.n_out + r.off
        return self.arena[at:at + r.rows * r.cols].view(r.rows, r.cols)

    def finalise(self, work=None):
        """Close the layout: allocate, give every Ref its address and pack the job tables.  work: the address of dtw_work_bytes()
        bytes of the caller's (held with hold()); None: the plan allocates them."""
        self.arena = torch.empty(max(1, self.n_out + self.n_scratch), dtype=torch.float64, device=self.dev)
        self.twf = torch.empty(max(1, self.n_twf), dtype=torch.int64, device=self.dev)
        a0, w0 = self.arena.data_ptr(), self.twf.data_ptr()
        base = (a0, a0 + 8 * self.n_out)
        for r in self.refs:
            r.addr = base[r.seg] + 8 * r.off
        R = Ref      # (an operand's address, spelled out per field as in resolve(): a call per pointer is a third of this loop)
        self.raw = b"".join(_JOB.pack(kind, rows, c0, c1, src_rows, 0, a.addr if a.__class__ is R else a or 0, b.addr if b.__class__ is R else b or 0,
                                 lda, ldb, idx or 0, dst.addr if dst.__class__ is R else dst or 0, out)
                       for kind, rows, c0, c1, src_rows, a, b, lda, ldb, idx, dst, out in self.jobs[0] + self.jobs[1])
        self.table = (_cabi.StatJob * (len(self.raw) // _JOB.size)).from_buffer_copy(self.raw)
        self.probs = list((_cabi.DtwProblem * len(self.probs)).from_buffer_copy(b"".join(
            _PROBLEM.pack(org.addr + 8 * c0, trg.addr + 8 * c0, org.cols, trg.cols, org.rows, trg.rows, org.cols - c0, mcd,
                          aligned.addr if aligned else 0, w0 + 8 * twf, frames.addr, mean.addr if mean else frames.addr + 8 * trg.rows)
            for org, trg, c0, mcd, aligned, twf, frames, mean in self.probs)))
        self.dtw_work_bytes()
        if work is None:
            self.work = torch.empty(self.work_bytes, dtype=torch.uint8, device=self.dev)
            work = self.work.data_ptr()
        self.work_ptr = work

    def begin(self, pinned=False):
        """The first step: the job table goes to the device (pinned: from a pinned buffer, without waiting for the copy), and what
        the later steps pass to the library is put together, so that they only launch."""
        raw, self.raw = torch.from_numpy(np.frombuffer(self.raw, np.uint8).copy()), None
        if pinned:
            self.stage = torch.empty(raw.numel(), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
            self.stage.copy_(raw)
            raw = self.stage
        self.jdev = raw.to(self.dev, non_blocking=pinned)
        if len(self.table) or len(self.probs):      # the library OBJECT of the steps; they look its methods up when they run
            self._lib, self._stream = gru_vae._lib(), gru_vae._stream()
        # (before the first mark: with profiling on, host time between two marks counts as the later step's)
        self._stats, self._a0 = [(self.job_ptr(k), len(self.jobs[k - 1])) for k in (1, 2)], self.arena.data_ptr()
        self.mark(None)

    def job_ptr(self, phase):
        """the device address of the phase's first job: phase 2's table follows phase 1's"""
        return self.jdev.data_ptr() + (phase - 1) * len(self.jobs[0]) * C.sizeof(_cabi.StatJob)

    def stats(self, phase):
        ptr, n = self._stats[phase - 1]
        if n:
            self._lib.eval_stats(ptr, n, self._a0, self._stream)
        self.mark(("stats1", "stats2")[phase - 1])

    def dtw_work_bytes(self):
        """what cvae_dtw_batch needs for the alignments declared (asked of the library once: call it when all are)"""
        if self.work_bytes is None:
            self.work_bytes = gru_vae._lib().dtw_batch_work_bytes(len(self.probs), self.t1max, self.t2max) if self.probs else 0
        return self.work_bytes

    def dtw(self):
        if self.probs:
            self._lib.dtw_batch(self.probs, self.work_ptr, self.work_bytes, self._stream)
        self.mark("dtw")

    def results(self):
        return self.arena[:max(1, self.n_out)]

    # ---- profiling ---------------------------------------------------------------------------------------------------------------
    def mark(self, name):
        """With profiling on: an event here; times() adds the device time since the previous mark to `name`."""
        if self._ev is not None:
            ev = self._spare.pop() if self._spare else torch.cuda.Event(enable_timing=True)
            ev.record()
            self._ev.append((name, ev))

    def times(self):
        """{name: device milliseconds} of the marked steps; call when the stream has been waited for."""
        ms = {}
        for (_, e0), (name, e1) in zip(self._ev, self._ev[1:]):
            ms[name] = ms.get(name, 0.0) + e0.elapsed_time(e1)
        return ms
