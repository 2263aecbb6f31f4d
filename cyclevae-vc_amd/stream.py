"""Live conversion (the online form of stage 6): chunked sessions batched into stacked passes.

stage6.convert_* need the whole utterance before they start.  A StreamConverter takes frames as they arrive, for many callers at
once: every step() runs ONE stacked encoder pass and ONE stacked decoder pass over the sessions that can advance, each session as
a single-row cell over a window of its utterance (cvae_gru_rnn_forward_stacked_carry: ctx_before / ctx_after, draw_frame0 and a
carried h), so what a session receives is the unbroken offline pass of its frames bit for bit, however they were chunked and
whoever else was live.  Frames move between buffers through cvae_stream_move, one launch per purpose (append, compact, pack): the
launches of a step do not depend on the number of sessions.  DESIGN.md 4.6 has the buffer scheme, the advance rule and the
kernel-class rule.  HIP device tensors and modules only; no fallback.
"""
import torch

import _cabi
import gru_vae


def _reach(m):
    """Frames the conv front-end looks ahead / behind: its padding (ks^layers - 1) / 2."""
    return (m.kernel_size ** m.dilation_size - 1) // 2


def _up4(n):
    return (n + 3) // 4 * 4      # arena offsets in floats: every buffer starts on a 16-byte boundary


class _Session(object):
    def __init__(self, sid, slot, n_rows, draw_id):
        self.sid, self.slot, self.n_rows, self.draw_id = sid, slot, n_rows, draw_id
        self.pushed = self.enc_done = self.dec_done = 0      # absolute frame numbers (Python ints: a stream has no end)
        self.closed = self.lost = False                      # lost: advanced in a step that raised the range status (policy "raise")
        self.in_half = self.lat_half = self.he = self.hd = 0      # the half of each double buffer that holds the committed state
        self.in_base = self.lat_base = 0                     # frame number of the first frame kept in the input / latent half
        self.in_end = 0                                      # frames [in_base, in_end) are in the input half; [in_end, pushed) are staged
        self.staged = []                                     # (device tensor or None, first frame in the staging buffer, frames)


class StreamConverter(object):
    """sc = StreamConverter(model_encoder, model_decoder, y_in_pp, y_in_trg, lat_dim, max_sessions=8, hop=16, max_pending=64)

        sid = sc.open(codes, draw_id=0)    codes [n_rows, dec.in_dim - lat_dim]: one decoder row per code, all rows of a session share
                                           ONE sampling of its latent (cvmcep / cvmcep_src of decode_gru-cyclevae_gauss.py:304-305)
        sc.push(sid, frames)               [k, Cin], k >= 0; a CPU tensor (pinned or not) or a tensor on the converter's device
        sc.close(sid)                      no more frames will come
        out = sc.step()                    {sid: {"cv": [n_rows, m, Cout], "lat": [m_e, 2L], "done": bool}}: device tensors, valid
                                           until the next step(); sessions with nothing to report are left out

    A step advances the encoder of every live session by a_e = min(hop, pushed - enc_done - (0 if closed else reach_enc)) frames and
    then its decoder by a_d = min(hop, enc_done - dec_done - (0 if the encoder has finished else reach_dec)): a frame comes out
    latency_frames = reach_enc + reach_dec frames behind the newest one pushed.  A session whose decoder reaches its last frame is
    returned with done = True and its slot is free for the next open().  rows: decoder rows a session may have (n_rows <= rows);
    max_sessions * rows cells fit one pass (32 at most).  A converter whose passes never exceed 3 rows runs the word-exchange
    kernels; every other converter runs EVERY pass on the dataflow kernel, also when fewer than 4 rows are live (the pass is then
    padded with idle cells): the bits a session receives do not depend on who else is live.
    seed None: one Philox seed drawn at construction; a session opened with draw_id = d draws what the offline pair rows with draw
    id d draw (stage6._decode_pairs: pair q draws with 2 n q, its cvmcep_trg with 2 n q + n).  posterior: as stage6.convert_pairs.
    push() beyond max_pending frames the encoder has not consumed raises ValueError; a step that raises leaves every session as it
    was.  Under gru_vae.set_range_policy("retry") a step that raised status 7 is repeated on the fp32-operand kernels.  Under "raise"
    (the default) nothing is added to a step: the status shows at the check in front of the NEXT step(), which raises CvaeRangeError
    before it touches a session -- but the step that met the value is committed by then, and the sessions that advanced in it carry
    NaN / inf states: they are lost and must be closed and opened again (lost_sessions() names them)."""

    def __init__(self, model_encoder, model_decoder, y_in_pp, y_in_trg, lat_dim, max_sessions=8, hop=16, max_pending=64,
                 n_smpl_dec=1, seed=None, posterior="gauss", rows=1):
        self._Ld, self._clamp = _cabi.posterior_flags(posterior, lat_dim)
        if model_encoder.hidden_layers > 1 or model_decoder.hidden_layers > 1:
            raise NotImplementedError("hidden_layers=%d/%d: a stream carries single-layer states between its windows (as "
                                      "stage6.convert_pairs(window=...)); convert stacked networks offline"
                                      % (model_encoder.hidden_layers, model_decoder.hidden_layers))
        S, R, hop, P = int(max_sessions), int(rows), int(hop), int(max_pending)
        if S < 1 or R < 1 or hop < 1 or int(n_smpl_dec) < 1:
            raise ValueError("max_sessions, rows, hop and n_smpl_dec must be at least 1, got %r, %r, %r, %r" % (max_sessions, rows, hop, n_smpl_dec))
        if S * R > 32:
            raise ValueError("max_sessions x rows = %d x %d cells: a pass stacks at most 32 (CVAE_MAX_CELLS)" % (S, R))
        self.reach_enc, self.reach_dec = _reach(model_encoder), _reach(model_decoder)
        if P < max(hop, self.reach_enc + 1):
            raise ValueError("max_pending=%d: an open session must be able to hold hop = %d frames, and more than the encoder's reach "
                             "(%d)" % (P, hop, self.reach_enc))
        L = int(lat_dim)
        if model_encoder.out_dim != 2 * L or model_decoder.in_dim <= L:
            raise ValueError("lat_dim=%d: the encoder writes %d values per frame, the decoder reads %d"
                             % (L, model_encoder.out_dim, model_decoder.in_dim))
        p0 = next(model_encoder.parameters())
        gru_vae._need_cuda(p0, "StreamConverter(model_encoder)")
        gru_vae._need_cuda(next(model_decoder.parameters()), "StreamConverter(model_decoder)")
        self.enc, self.dec, self.dev = model_encoder, model_decoder, p0.device
        self.S, self.R, self.hop, self.max_pending, self.L = S, R, hop, P, L
        self.n = int(n_smpl_dec)
        self.seed = gru_vae._draw_seed() if seed is None else int(seed)
        self.latency_frames = self.reach_enc + self.reach_dec
        self.Cin, self.Co, self.ncode = model_encoder.in_dim, model_decoder.out_dim, model_decoder.in_dim - L
        self._dataflow = S * R > 3
        # a pass of ONE frame would leave the persistent kernels (their plan needs T > 1): the shortest pass has two steps, and a
        # cell that advances by less passes frames = a
        self.Tmax = Tm = max(hop, 2)
        self.capI = self.reach_enc + P                  # kept context + everything the encoder has not consumed
        self.capL = 2 * self.reach_dec + Tm             # kept context + the decoder's lag (<= reach_dec) + one encoder pass
        He, Hd, Cin, Co, L2 = model_encoder.hidden_units, model_decoder.hidden_units, self.Cin, self.Co, 2 * L
        self._in_w, self._lat_w = _up4(self.capI * Cin), _up4(self.capL * L2)
        self._pack_w = _up4(R * Tm * Co) + _up4(Tm * L2)
        off, at = {}, 0
        for name, size in (("in", S * 2 * self._in_w), ("lat", S * 2 * self._lat_w), ("h_enc", 2 * S * He), ("h_dec", 2 * S * R * Hd),
                           ("dec_out", S * R * Tm * Co), ("pack", S * self._pack_w), ("stage", S * P * Cin), ("codes", S * R * self.ncode),
                           ("ypp", L2), ("y_dec", S * R * Co), ("idle_in", Tm * max(Cin, L2)), ("idle_out", 3 * Tm * max(Co, L2)),
                           ("idle_y", Co)):
            off[name] = at
            at += _up4(size)
        # every buffer of every session lives in one arena that starts out as NaN: a frame read before it was written shows
        self.arena = torch.full((at,), float("nan"), dtype=torch.float32, device=self.dev)
        self._off, self._base = off, self.arena.data_ptr()
        self._He, self._Hd = He, Hd
        f = lambda t: t.detach().to(device=self.dev, dtype=torch.float32).reshape(-1)
        self._buf("ypp", L2).copy_(f(y_in_pp))
        # idle cells (_pad_cells): zero frames / zero latent statistics and code in, their output next to it
        self._buf("idle_in", Tm * max(Cin, L2)).zero_()
        self._y_trg = f(y_in_trg)
        if self._y_trg.numel() != Co:
            raise ValueError("y_in_trg has %d values, the decoder writes %d" % (self._y_trg.numel(), Co))
        self._buf("idle_y", Co).copy_(self._y_trg)
        # Host pushes collect in a pinned staging buffer that a step sends in ONE asynchronous copy.  step() does not wait for the
        # device, so the copy may still be pending when the next push arrives: two buffers alternate, an event is recorded behind
        # each copy, and the first push into a buffer waits for the copy that last read it (two steps back: as a rule long done).
        self._stage_bufs = [torch.empty(S * P, Cin, dtype=torch.float32) for _ in range(2)]
        if self.dev.type == "cuda":
            self._stage_bufs = [b.pin_memory() for b in self._stage_bufs]
        self._stage_events = [None, None]      # behind the last copy out of each buffer (None: nothing pending)
        self._stage_cur = self._stage_used = 0
        lib = gru_vae._lib()
        self._de, self._ie = model_encoder.prepared(self.dev)
        self._dd, self._id = model_decoder.prepared(self.dev)
        self._ws_enc = torch.empty(lib.pass_workspace_bytes(self._de, max(S, 4), Tm), dtype=torch.uint8, device=self.dev)
        self._ws_dec = torch.empty(lib.pass_workspace_bytes(self._dd, max(S * R, 4), Tm), dtype=torch.uint8, device=self.dev)
        self._sessions, self._free, self._next_sid = {}, list(range(S)), 0
        self._last_advanced = set()      # sessions that advanced in the last committed step

    # -- the arena --------------------------------------------------------------------------------------------------------------
    def _buf(self, name, n, at=0):
        o = self._off[name] + at
        return self.arena[o:o + n]

    def _ptr(self, name, at=0):
        return self._base + 4 * (self._off[name] + at)

    def _in_ptr(self, s, half, frame=0):
        return self._ptr("in", (2 * s.slot + half) * self._in_w + frame * self.Cin)

    def _lat_ptr(self, s, half, frame=0):
        return self._ptr("lat", (2 * s.slot + half) * self._lat_w + frame * 2 * self.L)

    def _pad_cells(self, decoder, pins, ys, hi, outs, hl):
        """A converter of the dataflow class never runs a pass of fewer than four rows: three or fewer would take the word-exchange
        kernels, whose last bit differs.  Idle cells fill up: fresh single-row cells over zero frames that write to a scratch area."""
        lib = gru_vae._lib()
        for k in range(4 - len(pins) if self._dataflow else 0):
            if decoder:
                pins.append(lib.pass_input((self._ptr("idle_in"), self.ncode, 0), lat=self._ptr("idle_in"), lat_dim=self._Ld, seed=self.seed,
                                           n_draws=self.n))
            else:
                pins.append(lib.pass_input((self._ptr("idle_in"), self.Cin, self.Cin)))
            ys.append(self._ptr("idle_y") if decoder else self._ptr("ypp"))
            hi.append(None)
            hl.append(None)
            outs.append(self._ptr("idle_out", k * self.Tmax * max(self.Co, 2 * self.L)))

    # -- sessions ---------------------------------------------------------------------------------------------------------------
    def open(self, codes, draw_id=0, y_in=None):
        """codes [n_rows, dec.in_dim - lat_dim]; y_in: None (y_in_trg for every row) or [n_rows, Cout], the rows' first feedback
        (cvmcep_src starts from y_in_src).  Returns the session id."""
        c = torch.as_tensor(codes, dtype=torch.float32).reshape(-1, self.ncode)
        nr = c.shape[0]
        if not 1 <= nr <= self.R:
            raise ValueError("a session of this converter has 1..%d decoder rows (rows=%d), got %d" % (self.R, self.R, nr))
        if not self._free:
            raise RuntimeError("all %d sessions of this converter are open" % self.S)
        if int(draw_id) < 0:
            raise ValueError("draw_id must not be negative, got %r" % (draw_id,))
        y = self._y_trg.repeat(nr) if y_in is None else torch.as_tensor(y_in, dtype=torch.float32).reshape(-1)
        if y.numel() != nr * self.Co:
            raise ValueError("y_in has %d values for %d rows of %d" % (y.numel(), nr, self.Co))
        slot = self._free.pop(0)
        self._buf("codes", nr * self.ncode, slot * self.R * self.ncode).copy_(c.reshape(-1))
        self._buf("y_dec", nr * self.Co, slot * self.R * self.Co).copy_(y)
        sid = self._next_sid
        self._next_sid += 1
        self._sessions[sid] = _Session(sid, slot, nr, int(draw_id))
        return sid

    def _session(self, sid):
        s = self._sessions.get(sid)
        if s is None:
            raise KeyError("no open session %r" % (sid,))
        return s

    def push(self, sid, frames):
        """frames [k, Cin], k >= 0.  A host tensor is copied to the converter's staging buffer (the next step sends the whole buffer
        in one copy); a tensor on the converter's device is read in place by the next step, behind the current stream."""
        s = self._session(sid)
        if s.lost:
            raise RuntimeError("session %r is lost: it advanced in a step that met a value outside the range of the exact-operand "
                               "kernels (CvaeRangeError); close it and open a new one" % (sid,))
        if s.closed:
            raise RuntimeError("session %r is closed" % (sid,))
        if frames.dim() != 2 or frames.shape[1] != self.Cin:
            raise ValueError("push takes [k, %d] frames, got %s" % (self.Cin, tuple(frames.shape)))
        k = frames.shape[0]
        if k == 0:
            return
        if s.pushed + k - s.enc_done > self.max_pending:
            raise ValueError("session %r would hold %d frames the encoder has not consumed: max_pending=%d (step() first)"
                             % (sid, s.pushed + k - s.enc_done, self.max_pending))
        if frames.is_cuda:
            if frames.device != self.dev:
                raise ValueError("push: frames on %s, the converter runs on %s" % (frames.device, self.dev))
            s.staged.append((frames.detach().to(torch.float32).contiguous(), 0, k))
        else:
            ev = self._stage_events[self._stage_cur]
            if ev is not None:      # (the copy of two steps ago still reads this buffer)
                ev.synchronize()
                self._stage_events[self._stage_cur] = None
            self._stage_bufs[self._stage_cur][self._stage_used:self._stage_used + k].copy_(frames.detach())
            s.staged.append((None, self._stage_used, k))
            self._stage_used += k
        s.pushed += k

    def close(self, sid):
        s = self._session(sid)
        s.closed = True
        if s.lost:      # nothing more will come out of it: the slot is free at once
            del self._sessions[sid]
            self._free.append(s.slot)
            self._free.sort()

    def lost_sessions(self):
        """Sessions that advanced in a step whose range status a later check raised (policy "raise"): their carried states are NaN /
        inf.  step() leaves them out and push() refuses them; close() frees their slots."""
        return sorted(sid for sid, s in self._sessions.items() if s.lost)

    # -- a step -----------------------------------------------------------------------------------------------------------------
    def step(self):
        try:
            gru_vae.check_status()
        except _cabi.CvaeRangeError:
            for sid in self._last_advanced:
                if sid in self._sessions:
                    self._sessions[sid].lost = True
            self._last_advanced = set()
            raise
        if not self._sessions:
            return {}
        plan = gru_vae._with_range_retry(self._enqueue)
        return self._commit(plan)

    def _enqueue(self):
        """Everything a step puts on the current stream.  Reads the sessions, changes none of them: what it writes lies in the halves
        that do NOT hold the committed state (or behind the committed frames), so a step that fails, or that the range policy
        repeats, starts from the same state.  Returns what _commit applies."""
        lib, st = gru_vae._lib(), gru_vae._stream()
        Cin, L2, Co, Tm = self.Cin, 2 * self.L, self.Co, self.Tmax
        live = sorted((s for s in self._sessions.values() if not s.lost), key=lambda s: s.slot)
        new = {}
        # 1. compact: the last `reach` consumed frames plus everything not consumed go to the other half (never an overlap)
        jobs = []
        for s in live:
            v = new[s.sid] = {"in_half": s.in_half, "in_base": s.in_base, "lat_half": s.lat_half, "lat_base": s.lat_base}
            keep = max(0, s.enc_done - self.reach_enc)
            if keep > s.in_base:
                jobs.append(_cabi.MoveJob(self._in_ptr(s, 1 - s.in_half), self._in_ptr(s, s.in_half, keep - s.in_base),
                                          s.in_end - keep, Cin, Cin, Cin))
                v["in_half"], v["in_base"] = 1 - s.in_half, keep
            keep = max(0, s.dec_done - self.reach_dec)
            if keep > s.lat_base:
                jobs.append(_cabi.MoveJob(self._lat_ptr(s, 1 - s.lat_half), self._lat_ptr(s, s.lat_half, keep - s.lat_base),
                                          s.enc_done - keep, L2, L2, L2))
                v["lat_half"], v["lat_base"] = 1 - s.lat_half, keep
        lib.stream_move(jobs, st)
        # 2. append what was pushed since the last committed step: one copy of the staging buffer, one launch
        if self._stage_used:
            self._buf("stage", self._stage_used * Cin).view(-1, Cin).copy_(self._stage_bufs[self._stage_cur][:self._stage_used], non_blocking=True)
        jobs = []
        for s in live:
            v, at = new[s.sid], s.in_end
            for t, first, k in s.staged:
                src = self._ptr("stage", first * Cin) if t is None else t.data_ptr()
                jobs.append(_cabi.MoveJob(self._in_ptr(s, v["in_half"], at - v["in_base"]), src, k, Cin, Cin, Cin))
                at += k
            assert at == s.pushed and at - v["in_base"] <= self.capI, (at, s.pushed, v["in_base"], self.capI)
        lib.stream_move(jobs, st)
        # 3. the encoder cells
        flags = gru_vae._flags()
        cells = []
        for s in live:
            a = max(0, min(self.hop, s.pushed - s.enc_done - (0 if s.closed else self.reach_enc)))
            new[s.sid]["a_e"] = a
            if a:
                cells.append((s, a))
        if cells:
            T = max(2, max(a for _, a in cells))
            pins, ys, hi, outs, hl = [], [], [], [], []
            for s, a in cells:
                v = new[s.sid]
                assert s.enc_done - v["lat_base"] + T <= self.capL, (s.enc_done, v["lat_base"], T, self.capL)
                pins.append(lib.pass_input((self._in_ptr(s, v["in_half"], s.enc_done - v["in_base"]), Cin, Cin), frames=a,
                                           ctx_before=min(s.enc_done, self.reach_enc), ctx_after=min(s.pushed - s.enc_done - a, self.reach_enc)))
                ys.append(self._ptr("ypp") if s.enc_done == 0 else None)
                hi.append(None if s.enc_done == 0 else self._ptr("h_enc", (s.he * self.S + s.slot) * self._He))
                hl.append(self._ptr("h_enc", ((1 - s.he) * self.S + s.slot) * self._He))
                # (straight into the session's latent buffer; a cell shorter than the pass also writes T - a frames it will write again)
                outs.append(self._lat_ptr(s, v["lat_half"], s.enc_done - v["lat_base"]))
            self._pad_cells(False, pins, ys, hi, outs, hl)
            lib.gru_rnn_forward_stacked_carry(self._de, self._ie.data_ptr(), pins, ys, hi, 1, T, self._clamp, outs, hl,
                                              self._ws_enc.data_ptr(), self._ws_enc.numel(), flags, st)
        # 4. the decoder cells, behind the encoder pass of this step
        dcells = []
        for s in live:
            v = new[s.sid]
            e1 = s.enc_done + v["a_e"]
            fin = s.closed and e1 == s.pushed
            a = max(0, min(self.hop, e1 - s.dec_done - (0 if fin else self.reach_dec)))
            v["a_d"], v["k0"] = a, len(dcells)
            v["done"] = fin and s.dec_done + a == s.pushed
            if a:
                dcells += [(s, r, a, e1) for r in range(s.n_rows)]
        if dcells:
            T = max(2, max(c[2] for c in dcells))
            pins, ys, hi, outs, hl = [], [], [], [], []
            for k, (s, r, a, e1) in enumerate(dcells):
                v, row = new[s.sid], s.slot * self.R + r
                pins.append(lib.pass_input((self._ptr("codes", row * self.ncode), self.ncode, 0),
                                           lat=self._lat_ptr(s, v["lat_half"], s.dec_done - v["lat_base"]), lat_dim=self._Ld, seed=self.seed,
                                           draw_id=s.draw_id, frames=a, n_draws=self.n, ctx_before=min(s.dec_done, self.reach_dec),
                                           ctx_after=min(e1 - s.dec_done - a, self.reach_dec), draw_frame0=s.dec_done))
                ys.append(self._ptr("y_dec", row * Co) if s.dec_done == 0 else None)
                hi.append(None if s.dec_done == 0 else self._ptr("h_dec", (s.hd * self.S * self.R + row) * self._Hd))
                hl.append(self._ptr("h_dec", ((1 - s.hd) * self.S * self.R + row) * self._Hd))
                outs.append(self._ptr("dec_out", k * Tm * Co))
            self._pad_cells(True, pins, ys, hi, outs, hl)
            lib.gru_rnn_forward_stacked_carry(self._dd, self._id.data_ptr(), pins, ys, hi, 1, T, -1, outs, hl,
                                              self._ws_dec.data_ptr(), self._ws_dec.numel(), flags, st)
        # 5. pack what the step produced: per session [n_rows][a_d][Co] and [a_e][2L], contiguous
        jobs = []
        for s in live:
            v = new[s.sid]
            at = s.slot * self._pack_w
            v["cv_at"], v["lat_at"] = at, at + _up4(self.R * Tm * Co)
            for r in range(s.n_rows if v["a_d"] else 0):
                jobs.append(_cabi.MoveJob(self._ptr("pack", at + r * v["a_d"] * Co), self._ptr("dec_out", (v["k0"] + r) * Tm * Co),
                                          v["a_d"], Co, Co, Co))
            if v["a_e"]:
                jobs.append(_cabi.MoveJob(self._ptr("pack", v["lat_at"]), self._lat_ptr(s, v["lat_half"], s.enc_done - v["lat_base"]),
                                          v["a_e"], L2, L2, L2))
        lib.stream_move(jobs, st)
        return new

    def _commit(self, new):
        """The step is on the stream: the sessions move on.  Nothing here can fail."""
        out = {}
        self._last_advanced = {sid for sid, v in new.items() if v["a_e"] or v["a_d"]}
        for sid, v in new.items():
            s = self._sessions[sid]
            s.in_half, s.in_base, s.lat_half, s.lat_base = v["in_half"], v["in_base"], v["lat_half"], v["lat_base"]
            s.in_end, s.staged = s.pushed, []
            if v["a_e"]:
                s.enc_done += v["a_e"]
                s.he = 1 - s.he
            if v["a_d"]:
                s.dec_done += v["a_d"]
                s.hd = 1 - s.hd
            if v["a_e"] or v["a_d"] or v["done"]:
                out[sid] = {"cv": self._buf("pack", s.n_rows * v["a_d"] * self.Co, v["cv_at"]).view(s.n_rows, v["a_d"], self.Co),
                            "lat": self._buf("pack", v["a_e"] * 2 * self.L, v["lat_at"]).view(v["a_e"], 2 * self.L), "done": v["done"]}
            if v["done"]:
                del self._sessions[sid]
                self._free.append(s.slot)
                self._free.sort()
        if self._stage_used:      # the staging buffer rests until everything enqueued so far -- its copy included -- is through
            if self.dev.type == "cuda":
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(self.dev))
                self._stage_events[self._stage_cur] = ev
            self._stage_cur, self._stage_used = 1 - self._stage_cur, 0
        return out
