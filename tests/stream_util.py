"""Shared by tests/test_stream_cpu.py (host-fiber emulator, CPU tensors) and tests/test_stream_gpu.py (MI355X): the cases of
cvae_stream_move and of stream.StreamConverter.

Every comparison is bit for bit (np.array_equal): the yardstick is the unbroken offline path the goldens pin --
stage6.convert_pairs with the same seed and draw ids, in the same kernel class: a converter of at most three rows against ONE
offline pair (word-exchange kernels: 2 encoder / 3 decoder rows), a converter with max_sessions >= 4 against an offline call of at
least two pairs (dataflow kernel: >= 4 / >= 6 rows).  No tolerance is involved anywhere.

How utterances map to offline rows (stage6._decode_pairs): pair q = (utterance 2q, utterance 2q + 1), n = n_smpl_dec;
    utterance 2q      trg code, draw id 2nq      -> cvmcep of pair q;  with a second row (src code, y_in_src) -> cvmcep_src
    utterance 2q + 1  trg code, draw id 2nq + n  -> cvmcep_trg of pair q
and "lat" is the pair's lat_src / lat_trg.  An odd utterance at the end is paired with itself."""
import numpy as np
import torch

import _cabi
import synth

TRG_CODE, SRC_CODE = [0.0, 1.0], [1.0, 0.0]      # (decode_gru-cyclevae_gauss.py:309-314)
SEED = 20190721


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


# ---- cvae_stream_move ---------------------------------------------------------------------------------------------------------

def _stream_handle(dev):
    return torch.cuda.current_stream().cuda_stream if dev.type == "cuda" else 0


class MoveArena(object):
    """Sources and a NaN-filled destination arena on `dev`, the jobs laid out one after the other with guard floats between them, and
    the arena the jobs must leave (numpy)."""

    def __init__(self, dev, n_src=8192, n_dst=400000):
        self.dev = dev
        self.src_np = synth.normal("stream/move/src", (n_src,))
        self.src = t(self.src_np, dev)
        self.dst = torch.full((n_dst,), float("nan"), dtype=torch.float32, device=dev)
        self.want = np.full((n_dst,), np.nan, np.float32)
        self.at = 8
        assert self.src.data_ptr() % 16 == 0 and self.dst.data_ptr() % 16 == 0

    def job(self, rows, width, dst_stride, src_stride, dst_off=0, src_off=0):
        """One job: its destination starts at the next 16-byte boundary of the arena + dst_off floats, its source at float
        4 * (job number % 7) + src_off of the source array."""
        d0 = (self.at + 3) // 4 * 4 + dst_off
        s0 = 4 * (d0 % 7) + src_off
        assert s0 + max(rows - 1, 0) * src_stride + width <= self.src_np.size
        for r in range(rows):
            self.want[d0 + r * dst_stride:d0 + r * dst_stride + width] = self.src_np[s0 + r * src_stride:s0 + r * src_stride + width]
        self.at = d0 + max(rows - 1, 0) * dst_stride + width + 5
        assert self.at < self.want.size
        return _cabi.MoveJob(self.dst.data_ptr() + 4 * d0, self.src.data_ptr() + 4 * s0, rows, width, dst_stride, src_stride)

    def check(self, what):
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        got = self.dst.cpu().numpy()
        assert np.array_equal(got, self.want, equal_nan=True), (what, int((~((got == self.want) | (np.isnan(got) & np.isnan(self.want)))).sum()))


def check_move_shapes(lib, dev):
    """Widths 1, 3, 4, 54, 65; strides equal to the width, larger by 3 (misaligned rows) and the next multiple of 4 + 4 (aligned rows: the
    16-byte path with its 0-, 1- and 2-float tails); rows 0, 1, 37; pointers at 16 bytes and 1 float off on either side -- as ONE
    call of 180 jobs (two launches), into a NaN arena that must hold the jobs' rows and nothing else."""
    A = MoveArena(dev)
    jobs = []
    for width in (1, 3, 4, 54, 65):
        for stride in (width, width + 3, (width + 3) // 4 * 4 + 4):
            for rows in (0, 1, 37):
                for d_off, s_off in ((0, 0), (1, 0), (0, 1), (1, 1)):
                    jobs.append(A.job(rows, width, stride, stride if rows != 1 else stride + 4, d_off, s_off))
    assert len(jobs) == 180
    lib.stream_move(jobs, _stream_handle(dev))
    A.check("180 jobs")


def check_move_split(lib, dev, njobs):
    """1, 96 (one full launch) and 97 jobs (the split): jobs of 1 .. 5 rows of 6 floats, a rows == 0 job among them."""
    A = MoveArena(dev)
    jobs = [A.job(0 if q == 3 else 1 + q % 5, 6, 8, 6 + q % 3, q % 2, q % 3 == 1) for q in range(njobs)]
    lib.stream_move(jobs, _stream_handle(dev))
    A.check("%d jobs" % njobs)
    lib.stream_move([], _stream_handle(dev))       # an empty list is legal: a step with nothing to compact
    A.check("no jobs")


def check_move_refusals(lib, dev, raises):
    """The three refusals, each behind a good job in the same call: -1 with a message, and NOTHING enqueued (the good job did not
    run either)."""
    A = MoveArena(dev)
    base, src = A.dst.data_ptr(), A.src.data_ptr()
    good = _cabi.MoveJob(base + 4 * 64, src, 4, 6, 8, 6)
    bad = {
        "null pointer": [_cabi.MoveJob(None, src, 2, 4, 4, 4), _cabi.MoveJob(base, None, 2, 4, 4, 4)],
        "negative": [_cabi.MoveJob(base, src, -1, 4, 4, 4), _cabi.MoveJob(base, src, 2, -4, 4, 4), _cabi.MoveJob(base, src, 2, 4, -4, 4),
                     _cabi.MoveJob(base, src, 2, 4, 4, -4)],
        "exceeds a row stride": [_cabi.MoveJob(base, src, 2, 5, 4, 8), _cabi.MoveJob(base, src, 2, 5, 8, 4)],
        "overlap": [_cabi.MoveJob(base, base, 2, 4, 4, 4), _cabi.MoveJob(base + 4 * 7, base, 2, 4, 4, 4),      # 7 < (2 - 1) * 4 + 4 floats
                    _cabi.MoveJob(base, base + 4 * 11, 3, 4, 4, 4)],
    }
    for msg, cases in bad.items():
        for j in cases:
            with raises(_cabi.CvaeError, match=msg):
                lib.stream_move([good, j], _stream_handle(dev))
    A.check("refused calls")
    # neighbours that only touch are no overlap; null pointers with rows == 0 are legal
    lib.stream_move([_cabi.MoveJob(base + 4 * 8, base, 2, 4, 4, 4), _cabi.MoveJob(None, None, 0, 4, 4, 4)], _stream_handle(dev))


# ---- StreamConverter ----------------------------------------------------------------------------------------------------------

def module(gru_vae, sd, i, o, hidden, enc, dev, ks=3, ds=2):
    m = gru_vae.GRU_RNN(in_dim=i, out_dim=o, hidden_units=hidden, kernel_size=ks, dilation_size=ds, scale_in_flag=enc, scale_out_flag=not enc)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(dev).eval()


class Setup(object):
    """Networks of one synthetic problem on `dev` and utterances of the given lengths (H64 problem unless told otherwise: in 10,
    lat 4, out 6, hidden 64).  enc_ds / dec_ds: front-end depths (dilation_size) of the two networks."""

    def __init__(self, gru_vae, dev, lens, tag="stream", in_dim=10, out_dim=6, lat_dim=4, hidden=64, ks=3, enc_ds=2, dec_ds=2,
                 enc_sd=None):
        """enc_sd: None, or a function of the problem that returns the encoder's state dict (range_util.scaled_encoder)."""
        self.gru_vae, self.dev, self.lens, self.L = gru_vae, dev, list(lens), lat_dim
        Tm = max(lens)
        P = self.P = synth.CycleVAEProblem(B=len(lens), T=Tm, in_dim=in_dim, out_dim=out_dim, lat_dim=lat_dim, hidden=hidden, bias_scale=0.05,
                                           tag=tag, dilation_size=enc_ds, kernel_size=ks)
        dec_sd = P.dec
        if dec_ds != enc_ds:
            dec_sd = synth.CycleVAEProblem(B=1, T=1, in_dim=in_dim, out_dim=out_dim, lat_dim=lat_dim, hidden=hidden, bias_scale=0.05,
                                           tag=tag, dilation_size=dec_ds, kernel_size=ks).dec
        self.enc = module(gru_vae, enc_sd(P) if enc_sd else P.enc, in_dim, 2 * lat_dim, hidden, True, dev, ks, enc_ds)
        self.dec = module(gru_vae, dec_sd, lat_dim + 2, out_dim, hidden, False, dev, ks, dec_ds)
        self.utts = [np.ascontiguousarray(P.x[i, :n]) for i, n in enumerate(lens)]
        self.ypp = t(P.y_in_enc[:1], dev)
        self.yt = t(P.y_in_dec[:1], dev)
        self.ys = t(P.y_in_dec[:1] * 0.5 + 0.25, dev)      # (a different first feedback for the src-code row)
        self._offline = {}

    def offline(self, n=1, posterior="gauss", dataflow=False):
        """stage6.convert_pairs over the utterances paired as the module docstring says (computed once per argument set, never
        changed): a list per utterance of {"cv", "cv_src" (even utterances), "lat"} numpy arrays.  dataflow False: every pair in a
        call of its own (2 encoder / 3 decoder rows: the word-exchange kernels; each call numbers its pair 0); True: all pairs, at
        least two, in ONE call (the dataflow kernel)."""
        key = (n, posterior, dataflow)
        if key not in self._offline:
            import stage6
            u = [t(x, self.dev) for x in self.utts]
            pairs = [(u[2 * q], u[min(2 * q + 1, len(u) - 1)]) for q in range((len(u) + 1) // 2)]
            if dataflow and len(pairs) < 2:
                pairs.append(pairs[-1])
            res = []
            with torch.no_grad():
                for call in ([pairs] if dataflow else [[p] for p in pairs]):
                    res += stage6.convert_pairs(self.enc, self.dec, call, self.ypp, self.ys, self.yt, self.L, n_smpl_dec=n, seed=SEED,
                                                posterior=posterior)
            self.gru_vae.check_status(sync=True)
            out = []
            for i in range(len(u)):
                r = [v.cpu().numpy().copy() for v in res[i // 2]]
                out.append({"cv": r[0], "cv_src": r[1], "lat": r[3]} if i % 2 == 0 else {"cv": r[2], "lat": r[4]})
            self._offline[key] = out
        return self._offline[key]

    def draw_id(self, i, n=1, dataflow=False):
        return (2 * n * (i // 2) if dataflow else 0) + (n if i % 2 else 0)

    def converter(self, n=1, posterior="gauss", **kw):
        import stream
        return stream.StreamConverter(self.enc, self.dec, self.ypp, self.yt, self.L, n_smpl_dec=n, seed=SEED, posterior=posterior, **kw)


_SETUPS = {}


def setup(gru_vae, dev, lens, **kw):
    """Setup(...) once per argument set: the networks, the utterances and the offline results are shared by the tests of a process."""
    key = (str(dev), tuple(lens), tuple(sorted(kw.items())))
    if key not in _SETUPS:
        _SETUPS[key] = Setup(gru_vae, dev, lens, **kw)
    return _SETUPS[key]


def chunkings(n, hop, name):
    """The four ways of section 2 to feed n frames."""
    rnd = (1 + np.floor(synth.uniform01("stream/chunks/" + name, (n,)) * 20)).astype(int)
    out = {"all at once": [n], "single frames": [1] * n, "random 1..20": [], "larger than hop": []}
    left = n
    for k in rnd:
        if left <= 0:
            break
        out["random 1..20"].append(int(min(k, left)))
        left -= int(min(k, left))
    left = n
    while left > 0:
        out["larger than hop"].append(min(hop + 5, left))
        left -= out["larger than hop"][-1]
    assert all(sum(v) == n for v in out.values())
    return out


def run(sc, setup, plan, n=1, src_row=False, max_steps=2000, on_step=None, host_sync=True, device_pushes=True):
    """plan: list of dicts(utt=index, open=step, chunks=[...], close_after=steps between the last push and close()).  Every step of
    the loop opens the sessions that are due, pushes ONE chunk per open session (a chunk that would pass max_pending waits), closes
    the sessions whose last push lies close_after steps back, and calls sc.step().  Returns per plan entry {"cv": [rows, T, Co], "lat": [T, 2L], "steps": steps the
    session appeared in}, concatenated copies of what the steps returned.  host_sync False: the loop never waits for the device -- every
    step's output is cloned on the device and nothing is read back before the last step is enqueued (the host runs ahead, as a
    caller that hands the outputs to further device work does).  device_pushes: on the GPU the odd utterances are pushed as device
    tensors, the even ones from the host."""
    st = [dict(p, sid=None, left=list(p["chunks"]), at=0, cv=[], lat=[], steps=0, wait=p.get("close_after", 0), closed=False, done=False)
          for p in plan]
    for step in range(max_steps):
        for s in st:
            if s["sid"] is None and step >= s["open"]:
                codes = [TRG_CODE, SRC_CODE] if src_row else [TRG_CODE]
                y_in = torch.cat([setup.yt.reshape(1, -1), setup.ys.reshape(1, -1)]) if src_row else None
                s["sid"] = sc.open(torch.tensor(codes), draw_id=setup.draw_id(s["utt"], n, sc._dataflow), y_in=y_in)
            if s["sid"] is None or s["done"]:
                continue
            x = setup.utts[s["utt"]]
            if s["left"]:
                k = s["left"][0]
                try:
                    sc.push(s["sid"], t(x[s["at"]:s["at"] + k], setup.dev) if device_pushes and setup.dev.type == "cuda" and s["utt"] % 2 else
                            torch.from_numpy(x[s["at"]:s["at"] + k]))
                    s["left"].pop(0)
                    s["at"] += k
                except ValueError as e:
                    assert "max_pending" in str(e)
            if not s["left"] and not s["closed"]:      # (close_after = 0: closed in front of the step that follows the last push)
                if s["wait"] == 0:
                    sc.close(s["sid"])
                    s["closed"] = True
                s["wait"] -= 1
        out = sc.step()
        if on_step:
            on_step(step, out)
        for s in st:
            r = out.get(s["sid"]) if s["sid"] is not None and not s["done"] else None
            if r is not None:
                s["cv"].append(r["cv"].cpu().numpy().copy() if host_sync else r["cv"].clone())
                s["lat"].append(r["lat"].cpu().numpy().copy() if host_sync else r["lat"].clone())
                s["steps"] += 1
                s["done"] = r["done"]
        if all(s["done"] for s in st):
            break
    assert all(s["done"] for s in st), "sessions still open after %d steps" % max_steps
    setup.gru_vae.check_status(sync=True)
    if not host_sync:
        for s in st:
            s["cv"], s["lat"] = [v.cpu().numpy() for v in s["cv"]], [v.cpu().numpy() for v in s["lat"]]
    return [{"cv": np.concatenate(s["cv"], 1), "lat": np.concatenate(s["lat"], 0), "steps": s["steps"]} for s in st]


def same(got, want, what, src_row=False):
    n = want["lat"].shape[0]
    assert got["lat"].shape == want["lat"].shape and got["cv"].shape == ((2 if src_row else 1), n, want["cv"].shape[1]), \
        (what, got["lat"].shape, got["cv"].shape)
    assert np.isfinite(got["cv"]).all() and np.isfinite(got["lat"]).all(), what
    assert np.array_equal(got["lat"], want["lat"]), (what, "lat", float(np.abs(got["lat"] - want["lat"]).max()))
    assert np.array_equal(got["cv"][0], want["cv"]), (what, "cv", float(np.abs(got["cv"][0] - want["cv"]).max()))
    if src_row:
        assert np.array_equal(got["cv"][1], want["cv_src"]), (what, "cv_src", float(np.abs(got["cv"][1] - want["cv_src"]).max()))


def one_session(setup, chunks, utt=0, close_after=0, what="", n=1, posterior="gauss", src_row=False, max_sessions=1, **kw):
    """One session against its offline row: max_sessions = 1 is a word-exchange converter (one offline pair per call), max_sessions >= 4
    a dataflow converter with one live session (an offline call of at least two pairs)."""
    kw.setdefault("hop", 8)
    sc = setup.converter(n=n, posterior=posterior, max_sessions=max_sessions, rows=2 if src_row else 1, **kw)
    assert sc._dataflow == (max_sessions * (2 if src_row else 1) > 3)
    got = run(sc, setup, [dict(utt=utt, open=0, chunks=chunks, close_after=close_after)], n=n, src_row=src_row)[0]
    same(got, setup.offline(n, posterior, sc._dataflow)[utt], what or str(chunks), src_row)
    return got


MIX_LENS = (23, 17, 20, 9, 23)
MIX_OPEN = (0, 0, 1, 3, 3)


def mix_plan(lens=MIX_LENS, opens=MIX_OPEN, tag="mix"):
    """Section 5: random chunkings of 1..6 frames, closed 0..2 steps after the last push."""
    plan = []
    for i, (n, o) in enumerate(zip(lens, opens)):
        ks, left = [], n
        for k in (1 + np.floor(synth.uniform01("stream/%s/%d" % (tag, i), (n,)) * 6)).astype(int):
            if left <= 0:
                break
            ks.append(int(min(k, left)))
            left -= ks[-1]
        plan.append(dict(utt=i, open=o, chunks=ks, close_after=i % 3))
    return plan


def count_calls(sc_step):
    """Library calls (every method of _cabi.CvaeLib, by name) and torch copies (Tensor.copy_ / .to / .cpu / .cuda) made by one
    sc_step()."""
    import pytest
    calls, copies = {}, [0]
    with pytest.MonkeyPatch.context() as mp:
        for name in dir(_cabi.CvaeLib):
            fn = getattr(_cabi.CvaeLib, name)
            if name.startswith("_") or not callable(fn) or isinstance(_cabi.CvaeLib.__dict__.get(name), staticmethod):
                continue

            def wrapped(self, *a, _fn=fn, _name=name, **k):
                calls[_name] = calls.get(_name, 0) + 1
                return _fn(self, *a, **k)
            mp.setattr(_cabi.CvaeLib, name, wrapped)
        for name in ("copy_", "to", "cpu", "cuda", "clone", "contiguous"):
            def counted(self, *a, _fn=getattr(torch.Tensor, name), **k):
                copies[0] += 1
                return _fn(self, *a, **k)
            mp.setattr(torch.Tensor, name, counted)
        out = sc_step()
    return calls, copies[0], out


def check_host_runs_ahead(gv, dev, lens=(200, 190, 180, 170, 160), lag=None):
    """Five sessions pushed from the HOST and stepped with no wait for the device in between, behind `lag()` (on the GPU: a kernel
    that keeps the stream busy while the host enqueues everything): a staging buffer that a push rewrites before the step's copy
    has read it shows as wrong bits.  Every chunk differs from the one before it."""
    su = setup(gv, dev, lens, tag="ahead")
    want = su.offline(dataflow=True)
    sc = su.converter(max_sessions=5, hop=8, max_pending=16)
    plan = [dict(utt=i, open=0, chunks=[5] * (n // 5)) for i, n in enumerate(su.lens)]
    if lag:
        lag()
    got = run(sc, su, plan, host_sync=False, device_pushes=False)
    for i, g in enumerate(got):
        same(g, want[i], "host ahead, utterance %d" % i)
    assert sc._stage_cur in (0, 1) and min(g["steps"] for g in got) >= min(lens) // 8


def check_failed_step(gv, dev, monkeypatch):
    """The second pass call (the decoder's) of a step in mid-stream raises once: the sessions are what they were, and the step
    repeated -- and everything after it -- gives the offline bits."""
    su = setup(gv, dev, MIX_LENS + (14,), tag="mix")
    sc = su.converter(max_sessions=6, hop=4)
    lib = gv._lib()
    real, seen = lib.gru_rnn_forward_stacked_carry, [0]

    def failing(*a, **k):
        seen[0] += a[7] == -1      # (clamp_lat_dim: the decoder's pass)
        if a[7] == -1 and seen[0] == 3:
            seen[0] += 1
            raise _cabi.CvaeError("injected")
        return real(*a, **k)
    monkeypatch.setattr(lib, "gru_rnn_forward_stacked_carry", failing)
    state = lambda: {k: {f: (list(v) if f == "staged" else v) for f, v in vars(s).items()} for k, s in sc._sessions.items()}
    sid = sc.open(torch.tensor([TRG_CODE]))
    cv, lat, at, failed, done = [], [], 0, 0, False
    while not done:
        if at < 23:
            sc.push(sid, torch.from_numpy(su.utts[0][at:at + 6]))
            at += 6
        else:
            sc.close(sid)
        before = state()
        try:
            out = sc.step()
        except _cabi.CvaeError as e:
            assert "injected" in str(e)
            failed += 1
            assert state() == before and before[sid]["enc_done"] > 0 and len(before[sid]["staged"]) == 1
            out = sc.step()
            assert sc._sessions[sid].enc_done > before[sid]["enc_done"]
        cv.append(out[sid]["cv"].cpu().numpy().copy())
        lat.append(out[sid]["lat"].cpu().numpy().copy())
        done = out[sid]["done"]
    assert failed == 1
    same({"cv": np.concatenate(cv, 1), "lat": np.concatenate(lat, 0)}, su.offline(dataflow=True)[0], "through a failed step")


def check_range_policy(gv, dev, sink, raises):
    """The range fixture (scale_in of one channel x 1e5, tests/range_util.py) in a dataflow converter.  "retry": the step's output is
    the fp32-operand offline result.  "raise": the step returns; the check in front of the NEXT step raises CvaeRangeError before it
    touches a session, the session that advanced is marked lost (its carried state is NaN / inf), push refuses it, close frees its
    slot, and the converter goes on with the others.  sink: the status words the library writes (host memory)."""
    import range_util
    sync = (lambda: torch.cuda.synchronize()) if dev.type == "cuda" else (lambda: None)
    su = Setup(gv, dev, (20, 20, 20), tag="rng64", enc_sd=lambda P: range_util.scaled_encoder(P, 1e5))
    assert np.array_equal(su.P.x, range_util.problem("h64").x)
    gv.set_kernel("fp32")
    try:
        want = su.offline(dataflow=True)
    finally:
        gv.set_kernel("exact3")
    assert int(sink[3]) == 0
    plan = [dict(utt=i, open=0, chunks=[20]) for i in range(2)]
    prev = gv.set_range_policy("retry")
    try:
        got = run(su.converter(max_sessions=4, hop=32), su, plan)
    finally:
        gv.set_range_policy(prev)
    for i, g in enumerate(got):
        assert g["steps"] == 1
        same(g, want[i], "retry, utterance %d" % i)
    assert int(sink[3]) == 0
    sc = su.converter(max_sessions=4, hop=8)
    sid = sc.open(torch.tensor([TRG_CODE]))
    idle = sc.open(torch.tensor([TRG_CODE]))          # (pushes nothing: does not advance)
    sc.push(sid, torch.from_numpy(su.utts[0]))
    sc.step()
    sync()
    assert int(sink[3]) == _cabi.STATUS_RANGE
    before = {k: dict(vars(v), lost=None) for k, v in sc._sessions.items()}
    with raises(_cabi.CvaeRangeError):
        sc.step()
    assert {k: dict(vars(v), lost=None) for k, v in sc._sessions.items()} == before and sc.lost_sessions() == [sid]
    with raises(RuntimeError, match="lost"):
        sc.push(sid, torch.from_numpy(su.utts[0][:1]))
    assert sc.step() == {}                            # the lost session is left out: nothing raises the status again
    sync()
    assert int(sink[3]) == 0
    sc.close(sid)
    assert sid not in sc._sessions and idle in sc._sessions and len(sc._free) == 3
