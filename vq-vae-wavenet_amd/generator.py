"""Fast autoregressive generation: host-side mirror of Wavenet.build_generator
(wavenet.py:103-172) + the sampling loop of generate.py:103-113, running entirely on the GPU
through vqw_ar_decode_* / vqw_ar_wide_* (ring buffers instead of FIFO queues, on-device sampling).

FastGenerator (audio) and PriorGenerator (VQ codes) cut 1..8 rows into handles of the persistent kernel (or of the
launch-per-phase path) and share FastGenerator._run; WideGenerator and WidePriorGenerator run up to 1024 rows on one
vqw_ar_wide handle and share _WideBase._run and _WideBase._prefill.  What all four do alike (weight table, argument checks,
uniforms, per-row sampling settings, a prompt's checks and tail) is in the helpers in front of the classes.  Every public
method refuses in the order mode, sampling settings, tensor arguments, before anything touches the model or the device."""
import ctypes as C
import functools

import torch

from . import _lib as L


MAX_ROWS = 4    # batch rows of one persistent handle (its LDS budget); larger batches run as several handles
MAX_GROUP = 8   # handles of one launch (vqw_ar_decode_run_group_sampled_async)
CU_MARGIN = 8   # CUs left free when handles share a launch: a workgroup of a persistent grid that finds no free CU
#                 keeps its siblings spinning until their timeout (not applied to the whole-chip layout below, which is
#                 chosen only when it fits exactly and is what BASELINE.json configs[3] on one GPU asks for)


def sampling_settings(batch, mode, temperature=1.0, top_k=0, top_p=1.0):
    """Validate the sampling keywords of FastGenerator.generate / PriorGenerator.sample and broadcast them to one
    (temperature, top_k, top_p) per row.  Each keyword is a scalar (every row) or a sequence of `batch` values.
    temperature: finite, > 0 (1 = off); top_k: integer >= 0 (0 = off, >= the class count = off); top_p: in (0, 1] (1 = off).
    They apply to mode 'sample' only: a non-default setting with mode 'greedy' is refused.  Returns None when every row is
    at its defaults (the library is then handed no settings: the plain sampling, bit for bit), else a list of `batch` tuples."""
    import math

    def rows(name, v):
        if isinstance(v, (str, bytes)):
            raise ValueError('%s must be a number or a sequence of %d numbers' % (name, batch))
        if hasattr(v, 'tolist'):              # numpy / torch scalars and arrays
            v = v.tolist()
        if isinstance(v, (list, tuple)):
            if len(v) != batch:
                raise ValueError('%s: %d values for a batch of %d rows' % (name, len(v), batch))
            return list(v)
        return [v] * batch

    out = []
    for t, k, p in zip(rows('temperature', temperature), rows('top_k', top_k), rows('top_p', top_p)):
        if isinstance(t, bool) or not isinstance(t, (int, float)) or not math.isfinite(t) or t <= 0:
            raise ValueError('temperature must be finite and > 0 (got %r)' % (t,))
        if isinstance(k, bool) or not (isinstance(k, int) or (isinstance(k, float) and k.is_integer())) or k < 0:
            raise ValueError('top_k must be an integer >= 0 (got %r)' % (k,))
        if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0 < p <= 1:
            raise ValueError('top_p must be in (0, 1] (got %r)' % (p,))
        out.append((float(t), int(k), float(p)))
    default = all(t == 1.0 and k == 0 and p == 1.0 for t, k, p in out)
    if not default and mode != 'sample':
        raise ValueError('temperature / top_k / top_p apply to mode \'sample\' only (mode is %r)' % (mode,))
    return None if default else out


def pick_layout(batch, R, cus):
    """(rows per handle, channels per workgroup [0 = the library's choice]) of a batch.  Rows never interact
    (generate.py:40,103-113), so how they are grouped into handles is free.  Measured at the reference widths
    (tools/ar_layouts.py, us per step; profiles/round3_ar_layouts.txt):
        rows   one handle   one-row handles, 8 channels per workgroup (R/8 = 32 workgroups each), ONE launch
         1        65             --
         2       103             66
         4       127             94
         8   129 (2 x 4 rows)   118 (8 x 32 workgroups = every CU of the chip)
    One-row handles are independent pipelines: a handle's step time grows with its rows (every exchange carries B values per
    channel and every dot product is formed B times), and side by side they only share the fabric the exchanges cross.
      * up to MAX_GROUP rows that fit the chip as one-row handles: one row per handle, 8 channels per workgroup;
      * otherwise handles of up to MAX_ROWS rows (more rows per weight byte streamed: the better AGGREGATE rate once the rows
        no longer fit side by side), as many per launch as fit, the rest in further waves.
    VQW_AR_ROWS / VQW_AR_CPB override."""
    import os
    rows = cpb = None
    if os.environ.get('VQW_AR_ROWS'):
        rows = max(1, min(MAX_ROWS, int(os.environ['VQW_AR_ROWS'])))
    if os.environ.get('VQW_AR_CPB') in ('4', '8'):
        cpb = int(os.environ['VQW_AR_CPB'])
    if rows is None and cpb is None and 1 < batch <= MAX_GROUP and R % 8 == 0 and (R // 8) * batch <= cus:
        return 1, 8
    if rows is None:
        n_parts = -(-batch // MAX_ROWS)
        rows = -(-batch // n_parts)
    return rows, (cpb or 0)


def plan_rows(lengths, max_rows):
    """Group rows of the given lengths into batches for WideGenerator: rows sorted by length (ties by index), cut into
    consecutive batches of at most max_rows.  A batch runs for its longest row, so the steps its shorter rows are carried
    along for are padding.  Returns (batches, padded): batches a list of lists of row indices, the batches and the rows of
    each in ascending length; padded the sum over batches of (longest - own) over its rows.  Pure: no GPU, no model."""
    if isinstance(max_rows, bool) or not isinstance(max_rows, int) or max_rows < 1:
        raise ValueError('max_rows must be an integer >= 1 (got %r)' % (max_rows,))
    lengths = [int(n) for n in lengths]
    if any(n < 0 for n in lengths):
        raise ValueError('lengths must be >= 0')
    order = sorted(range(len(lengths)), key=lambda i: (lengths[i], i))
    batches = [order[i:i + max_rows] for i in range(0, len(order), max_rows)]
    padded = sum(lengths[b[-1]] - lengths[i] for b in batches for i in b)
    return batches, padded


def _weights_of(model, keep):
    """vqw_ar_weights over the model's LIVE variables; the ctypes arrays it points to are appended to `keep`."""
    P = model.P
    nl, R, S = model.L, model.R, model.S
    w = L.ArWeights()
    w.n_layers, w.kernel_size, w.R, w.S, w.Q, w.Cc, w.pre_k = nl, model.ks, R, S, model.Q, model.Cc, model.pre_k
    dil = (C.c_int32 * nl)(*model.dil)
    w.dilations = dil
    f4 = 4  # bytes per float

    def arr(ptrs):
        a = (C.c_void_p * nl)(*ptrs)
        return a
    gw = arr([P['gated_w'][l].data_ptr() for l in range(nl)])
    gb = arr([P['gated_b'][l].data_ptr() for l in range(nl)])
    cw = arr([P['cond_w'].data_ptr() + l * 2 * R * f4 for l in range(nl)])
    ow = arr([P['out_w'][l].data_ptr() for l in range(nl)])
    ob = arr([P['out_b'][l].data_ptr() for l in range(nl)])
    keep.extend([dil, gw, gb, cw, ow, ob])
    w.gated_w, w.gated_b, w.cond_w, w.out_w, w.out_b = gw, gb, cw, ow, ob
    w.cond_ld, w.out_ld = model.Mall, S + R
    w.pre_w, w.pre_b = P['pre_w'].data_ptr(), P['pre_b'].data_ptr()
    w.skip0_w, w.skip0_b = P['skip0_w'].data_ptr(), P['skip0_b'].data_ptr()
    w.post1_w, w.post1_b = P['post1_w'].data_ptr(), P['post1_b'].data_ptr()
    w.post1_cond_w, w.post1_cond_ld = P['cond_w'].data_ptr() + nl * 2 * R * f4, model.Mall
    w.post2_w, w.post2_b = P['post2_w'].data_ptr(), P['post2_b'].data_ptr()
    return w


def _sampling_rows(settings):
    """vqw_ar_sampling[len(settings)] of sampling_settings' tuples; None (NULL: every row at its defaults) for None."""
    if settings is None:
        return None
    rows = (L.ArSampling * len(settings))()
    for j, (t, k, p) in enumerate(settings):
        rows[j].temperature, rows[j].top_k, rows[j].top_p = t, min(k, 0x7fffffff), p
    return rows


def _check_mode(mode):
    if mode not in ('greedy', 'sample'):
        raise NotImplementedError('decode mode %s not implemented' % mode)   # utils.py:46


def _check_encoding(encoding, B, Cc):
    if (not isinstance(encoding, torch.Tensor) or encoding.dtype != torch.float32 or encoding.dim() != 3
            or encoding.shape[0] != B or encoding.shape[1] != Cc):
        raise ValueError('encoding must be a float32 [%d][%d][Tz] tensor' % (B, Cc))


def _check_speakers(spk, B):
    if spk.numel() != B:
        raise ValueError('%d speaker ids for a batch of %d' % (spk.numel(), B))


def _uniforms_of(uniforms, mode, B, n, dev, n_name):
    """The float32 [B][n] uniforms of mode 'sample', drawn here when None (np.random.rand in utils.py:22); None for 'greedy'."""
    if mode != 'sample':
        return None
    if uniforms is None:
        uniforms = torch.rand(B, n, device=dev)
    if uniforms.shape != (B, n) or uniforms.dtype != torch.float32:
        raise ValueError('uniforms must be float32 [B][%s]' % n_name)
    return uniforms


@functools.lru_cache(maxsize=None)
def _row_slices(parts):
    """parts: the rows of each handle (a tuple) -> the slice of the batch each handle owns."""
    starts = [sum(parts[:i]) for i in range(len(parts))]
    return tuple(slice(b0, b0 + nb) for b0, nb in zip(starts, parts))


PRIOR_RATIO = 64    # code steps per condition frame (prior.CODES_PER_FRAME)
PREFILL_BUDGET = 2 << 30    # bytes of workspace one teacher-forced pass of a wide prefill may take (prefill_chunk)


def prefill_chunk(batch, R, Mall, Tw, Tzw, budget=PREFILL_BUDGET):
    """Rows per teacher-forced pass of a wide prefill (WideGenerator.prefill_prompt, chunk_rows=None): the largest chunk whose
    pass workspace stays within `budget` bytes, at least 1, at most `batch`.  A pass over a window of Tw steps and Tzw condition
    frames (wavenet.prefill_window) holds per row two layer inputs and the gated tensor, [R][Tw] each, and the projected
    condition [Mall][Tzw]: 4 * (3 R Tw + Mall Tzw) bytes (25 MB at the reference widths with a saturated window, 19 MB of
    it the three [R][Tw] tensors, where 1024 rows at once would be 26 GB).  Pure: no GPU, no model."""
    for name, v in (('batch', batch), ('R', R), ('Mall', Mall)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError('prefill_chunk: %s must be an integer >= 1 (got %r)' % (name, v))
    if Tw < 0 or Tzw < 0 or budget < 0:
        raise ValueError('prefill_chunk: Tw, Tzw and budget must be >= 0 (got %r, %r, %r)' % (Tw, Tzw, budget))
    per_row = 4 * (3 * R * Tw + Mall * Tzw)
    return batch if per_row == 0 else max(1, min(batch, int(budget) // per_row))


def even_chunk(batch, max_rows):
    """The chunk that cuts `batch` rows into the fewest passes of at most max_rows rows, as evenly as they go:
    ceil(batch / ceil(batch / max_rows)).  256 rows at 85 per pass are 4 x 64, not 85 + 85 + 85 + 1: the same number of
    passes, none of one row.  Pure."""
    for name, v in (('batch', batch), ('max_rows', max_rows)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError('even_chunk: %s must be an integer >= 1 (got %r)' % (name, v))
    passes = -(-batch // max_rows)
    return -(-batch // passes)


def _check_prompt(prompt, encoding, B, Cc, ratio):
    """The argument checks of FastGenerator.prefill / WideGenerator.prefill_prompt; returns T, the prompt's length."""
    if not isinstance(prompt, torch.Tensor) or prompt.dtype != torch.float32 or prompt.dim() != 2 or prompt.shape[0] != B:
        raise ValueError('prompt must be a float32 [%d][T] tensor' % B)
    _check_encoding(encoding, B, Cc)
    T = prompt.shape[1]
    if T > encoding.shape[2] * ratio:
        raise ValueError('a prompt of %d samples is longer than the encoding (%d frames x %d)' % (T, encoding.shape[2], ratio))
    return T


def _check_codes(codes, spk, B, Q):
    """The argument checks of PriorGenerator.prefill / WidePriorGenerator.prefill_codes; returns T, the number of prompt codes."""
    if (not isinstance(codes, torch.Tensor) or codes.dtype != torch.int32 or codes.dim() != 2 or codes.shape[0] != B
            or not codes.is_cuda):
        raise ValueError('codes must be an int32 [%d][T] tensor on the GPU' % B)
    _check_speakers(spk, B)
    T = codes.shape[1]
    if T and (int(codes.min()) < 0 or int(codes.max()) >= Q):
        raise ValueError('codes must lie in [0, %d)' % Q)
    return T


def _prefill_tail(x, T, pre_k):
    """[B][pre_k]: the prompt's last pre_k values x[:, T - pre_k : T], zeros where that reaches before step 0 (ignored by the
    library): the tail of vqw_ar_decode_prefill_finish / vqw_ar_wide_prefill_finish."""
    n = min(T, pre_k)
    tail = torch.zeros(x.shape[0], pre_k, dtype=x.dtype, device=x.device)
    tail[:, pre_k - n:] = x[:, T - n:T]
    return tail


class _Closes:
    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _WideBase(_Closes):
    """One vqw_ar_wide handle (csrc/ar_wide.hip) over the model's LIVE variables, and one run of it.  A subclass says how its
    handle is created (_create) and what its public method hands to _run."""
    _n_name = 'n_steps'          # the step count's name in the subclass's public method (for the messages)

    def __init__(self, model, batch):
        self.model, self.B = model, batch
        self._keep = []
        self._w = _weights_of(model, self._keep)
        self._h = None
        h = C.c_void_p()
        self._create(h, self._w)
        self._h = h

    def reset(self):
        """sess.run(wavenet.init_ops) (generate.py:105): empty queues, the next sample is step 0."""
        L.check(L.lib().vqw_ar_wide_reset(self._h, L.stream()))

    def _prefill(self, x, cond, T, ratio, audio, chunk_rows):
        """reset, then the prompt's layer inputs into the rings, chunk_rows rows per teacher-forced pass (each pass's
        net[l] scattered by vqw_ar_wide_prefill_layer as soon as it is made), then the input history, the last value and the
        step counter (vqw_ar_wide_prefill_finish).  A row's pass does not see the other rows, so its state does not depend
        on the chunking.  chunk_rows None: prefill_chunk's choice for the prompt's window, cut evenly (even_chunk)."""
        from .wavenet import prefill_window
        if chunk_rows is not None and (isinstance(chunk_rows, bool) or not isinstance(chunk_rows, int) or chunk_rows < 1):
            raise ValueError('chunk_rows must be an integer >= 1 or None (got %r)' % (chunk_rows,))
        lib, st, m = L.lib(), L.stream(), self.model
        L.check(lib.vqw_ar_wide_reset(self._h, st))
        if T == 0:
            return
        _, s0, end = prefill_window(T, m.ks, m.dil, m.pre_k, ratio)
        if chunk_rows is None:
            chunk_rows = even_chunk(self.B, prefill_chunk(self.B, m.R, m.Mall, end - s0, (end - s0) // ratio))
        for r0 in range(0, self.B, chunk_rows):
            n = min(chunk_rows, self.B - r0)

            def sink(l, net, t0):
                L.check(lib.vqw_ar_wide_prefill_layer(self._h, l, L.ptr(net), net.shape[2], t0, T, r0, n, st))
            m.decoder_states(x[r0:r0 + n], cond[r0:r0 + n], T, sink, ratio)
        tail = _prefill_tail(x, T, m.pre_k)
        L.check(lib.vqw_ar_wide_prefill_finish(self._h, T, L.ptr(tail) if audio else None, None if audio else L.ptr(tail), st))

    def _run(self, cond, Tz, ratio, n, mode, uniforms, settings, audio, return_probs):
        """n steps of every row on condition cond [B][Cc][Tz]; audio [B][n] or None (code mode).  Returns (indices, probs of
        the last step or None)."""
        L.require_cuda(cond, uniforms)
        uniforms = _uniforms_of(uniforms, mode, self.B, n, cond.device, self._n_name)
        idx = torch.empty(self.B, n, dtype=torch.int32, device=cond.device)
        probs = torch.empty(self.B, self.model.Q, device=cond.device) if return_probs else None
        lib = L.lib()
        L.check(lib.vqw_ar_wide_run_async(self._h, L.ptr(cond), Tz, ratio, n, 0 if mode == 'greedy' else 1, L.ptr(uniforms),
                                          _sampling_rows(settings), L.ptr(audio), L.ptr(idx), L.ptr(probs), L.stream()))
        L.check(lib.vqw_ar_wide_wait(self._h))
        return idx, probs

    def close(self):
        if getattr(self, '_h', None) is not None:
            L.lib().vqw_ar_wide_destroy(self._h)
            self._h = None


class WideGenerator(_WideBase):
    """Generation for many rows at once (1..1024 per handle) on vqw_ar_wide_* (csrc/ar_wide.hip): every layer of a step is
    a GEMM over all rows on the exact-fp32 MFMA.  Built for throughput: converting a list of utterances (generate.py
    -audio_list); FastGenerator stays the right choice for one to eight rows.  Uses the model's LIVE variables, like
    FastGenerator.  A row's indices, audio and probabilities do not depend on the batch it ran in (its size, the row's
    position, the other rows), and a run cut into several generate() calls equals the single run bit for bit.

    The class has no prefill attribute, and that name stays FastGenerator's: a wide handle is prefilled in chunks of rows, by
    prefill_prompt(), which takes FastGenerator.prefill's arguments and meaning plus chunk_rows."""

    def _create(self, h, w):
        L.check(L.lib().vqw_ar_wide_create(C.byref(h), C.byref(w), self.B))
        if self.model.levels != 256:     # the model's mu-law level (a created handle compands at 256)
            L.check(L.lib().vqw_ar_wide_set_levels(h, self.model.levels))

    def prefill_prompt(self, prompt, encoding, ratio=None, chunk_rows=None):
        """FastGenerator.prefill for a wide handle: every row in the state of reset() and T = prompt.shape[1] steps
        teacher-forced on its prompt; the next generate() continues at step T.  prompt float32 [B][T] in [-1, 1] on the GPU;
        encoding [B][Cc][Tz], the one the later generate calls use, with Tz * ratio >= T.  T = 0 is reset().  The
        teacher-forced pass (VQVAE.decoder_states) runs over chunk_rows rows at a time (None: prefill_chunk's choice, which
        bounds the pass's workspace, cut evenly).  A row's state, and so its continuation, does not depend on chunk_rows,
        on the batch size, on the row's position or on the other rows, bit for bit."""
        ratio = ratio or 64
        T = _check_prompt(prompt, encoding, self.B, self.model.Cc, ratio)
        L.require_cuda(prompt.contiguous(), encoding.contiguous())
        self._prefill(prompt.contiguous(), encoding.contiguous(), T, ratio, True, chunk_rows)

    def generate(self, encoding, n_steps, mode='greedy', uniforms=None, ratio=None, return_probs=False,
                 temperature=1.0, top_k=0, top_p=1.0):
        """encoding [B][Cc][Tz] (model.encode); continues from the current queue state, sample i of the run using condition
        frame (steps so far + i) // ratio (the last frame beyond it).  temperature / top_k / top_p (mode 'sample' only;
        scalars or one value per row): see sampling_settings and vqw_ar_sampling in include/vqwave.h.
        Returns (audio [B][n] float32, indices [B][n] int32[, probs of the last step [B][Q]: the distribution sampled])."""
        _check_mode(mode)
        settings = sampling_settings(self.B, mode, temperature, top_k, top_p)
        _check_encoding(encoding, self.B, self.model.Cc)
        encoding = encoding.contiguous()
        audio = torch.empty(self.B, n_steps, device=encoding.device)
        idx, probs = self._run(encoding, encoding.shape[2], ratio or 64, n_steps, mode, uniforms, settings, audio, return_probs)
        return (audio, idx, probs) if return_probs else (audio, idx)


class WidePriorGenerator(_WideBase):
    """Samples VQ codes from a prior.LatentPrior for many rows at once (1..1024 per handle) on the wide generator's code-input
    mode (vqw_ar_wide_prior_create, csrc/ar_wide.hip): the input stage gathers rows of W_pre by the previous codes, the drawn
    index is the next input, everything between is WideGenerator's step.  Built for throughput: a corpus sampled from the
    prior (generate.py -prior -count M); PriorGenerator stays the right choice for one to eight rows.  Uses the prior's LIVE
    variables, read in place (prior.use_ema_weights() first for the EMA shadows).  A row's codes and probabilities do not
    depend on the batch it ran in, and a run cut into several sample() calls equals the single run bit for bit.

    The class has no prefill attribute, and that name stays PriorGenerator's: a wide handle is prefilled in chunks of rows, by
    prefill_codes(), which takes PriorGenerator.prefill's arguments and meaning plus chunk_rows."""
    _n_name = 'n_frames'

    def __init__(self, prior, batch):
        self._t = 0
        super().__init__(prior, batch)

    def _create(self, h, w):
        L.check(L.lib().vqw_ar_wide_prior_create(C.byref(h), C.byref(w), self.B, self.model.Q))

    def reset(self):
        """Empty history ("no code yet": a zero one-hot, not code 0); the next sample is step 0."""
        super().reset()
        self._t = 0

    def prefill_codes(self, codes, spk, chunk_rows=None):
        """PriorGenerator.prefill for a wide handle: every row in the state of reset() and T = codes.shape[1] steps
        teacher-forced on its codes; the next sample() continues at step T.  codes int32 [B][T] in [0, k) on the GPU, spk
        int64 [B] (the speakers the later sample calls use).  T = 0 is reset().  chunk_rows: as in WideGenerator.prefill_prompt."""
        T = _check_codes(codes, spk, self.B, self.model.Q)
        cond = self.model.speaker_condition(spk.contiguous(), max(1, -(-T // PRIOR_RATIO)))
        self._prefill(codes.contiguous(), cond, T, PRIOR_RATIO, False, chunk_rows)
        self._t = T

    def sample(self, n_frames, spk, mode='greedy', uniforms=None, return_probs=False, temperature=1.0, top_k=0, top_p=1.0):
        """n_frames codes per row, continuing from the current state.  spk int64 [B] on the GPU.  mode 'greedy' (argmax) or
        'sample' (searchsorted(cumsum(p), u) with uniforms [B][n_frames], drawn here when None; u above the cdf's last
        value gives the last code), tempered / truncated by temperature, top_k, top_p as in WideGenerator.generate.
        Returns codes int32 [B][n_frames][, probabilities of the last step [B][k]: the distribution sampled]."""
        _check_mode(mode)
        settings = sampling_settings(self.B, mode, temperature, top_k, top_p)
        _check_speakers(spk, self.B)
        Tz = -(-(self._t + n_frames) // PRIOR_RATIO)
        cond = self.model.speaker_condition(spk.contiguous(), Tz)
        idx, probs = self._run(cond, Tz, PRIOR_RATIO, n_frames, mode, uniforms, settings, None, return_probs)
        self._t += n_frames
        return (idx, probs) if return_probs else idx


class FastGenerator(_Closes):
    def __init__(self, model, batch):
        """Uses the model's LIVE variables (call model.use_ema_weights() first to mirror
        generate.py:88-90, which restores the EMA shadows).  Rows of the batch never interact
        (generate.py:40,103-113), so a batch is cut into independent handles (pick_layout); as many of them as the
        chip has CUs for (one resident workgroup per CU, R/4 or R/8 workgroups per handle) share ONE launch and
        generate side by side, the rest follow in further waves."""
        self.model, self.B = model, batch
        cus = torch.cuda.get_device_properties(model.dev).multi_processor_count
        rows, cpb = pick_layout(batch, model.R, cus)
        self._parts = [rows] * (batch // rows) + ([batch % rows] if batch % rows else [])
        self._keep = []
        self._w = _weights_of(model, self._keep)
        self._hs = []
        for nb in self._parts:
            h = C.c_void_p()
            self._create(h, self._w, nb, cpb)
            self._hs.append(h)
        # waves of handles that are co-resident by construction: floor((CUs - margin) / workgroups), at most MAX_GROUP
        # (no margin where the whole batch fits the chip exactly: the one-utterance-per-XCD layout)
        nwg = [L.lib().vqw_ar_decode_workgroups(h) for h in self._hs]
        whole = len(set(nwg)) == 1 and nwg[0] > 0 and len(self._hs) <= MAX_GROUP and nwg[0] * len(self._hs) <= cus
        self._waves, i = [], 0
        while i < len(self._hs):
            if nwg[i] <= 0:                      # launch-per-phase path: one handle at a time
                self._waves.append([i]); i += 1
                continue
            cap = max(1, min(MAX_GROUP, (cus - (0 if whole else CU_MARGIN)) // nwg[i]))
            j = i + 1
            while j < len(self._hs) and j - i < cap and nwg[j] == nwg[i] and (self._parts[j] > 1) == (self._parts[i] > 1):
                j += 1
            self._waves.append(list(range(i, j))); i = j

    def _create(self, h, w, rows, cpb):
        L.check(L.lib().vqw_ar_decode_create_ex(C.byref(h), C.byref(w), rows, cpb))
        if self.model.levels != 256:     # the model's mu-law level (a created handle compands at 256)
            L.check(L.lib().vqw_ar_decode_set_levels(h, self.model.levels))

    def reset(self):
        """sess.run(wavenet.init_ops) (generate.py:105)."""
        for h in self._hs:
            L.check(L.lib().vqw_ar_decode_reset(h, L.stream()))

    def prefill(self, prompt, encoding, ratio=None):
        """Leave every row in the state it would have after reset() and T = prompt.shape[1] steps teacher-forced on its prompt
        (the input of step t is mu_law_encode(prompt[t-1]), zero at t = 0): the next generate() continues at step T, sample T + i
        using condition frame (T + i) // ratio of the encoding it is given.  prompt float32 [B][T] in [-1, 1] on the GPU;
        encoding [B][Cc][Tz] (model.encode), the one the later generate calls use, with Tz * ratio >= T.  T = 0 is reset().
        One teacher-forced pass over at most model.prefill_window's window (VQVAE.decoder_states), scattered into the rings."""
        ratio = ratio or 64
        T = _check_prompt(prompt, encoding, self.B, self.model.Cc, ratio)
        L.require_cuda(prompt.contiguous(), encoding.contiguous())
        self._prefill(prompt.contiguous(), encoding.contiguous(), T, ratio, audio=True)

    def _prefill(self, x, cond, T, ratio, audio):
        """reset, then the prompt's layer inputs into every handle's rings (each handle its slice of the rows), then the input
        history and the step counter (vqw_ar_decode_prefill_layer / _finish)."""
        lib, st = L.lib(), L.stream()
        for h in self._hs:
            L.check(lib.vqw_ar_decode_reset(h, st))
        rows = _row_slices(tuple(self._parts))
        if T == 0:
            return
        x = x.contiguous()

        def sink(l, net, s0):
            for h, r in zip(self._hs, rows):
                L.check(lib.vqw_ar_decode_prefill_layer(h, l, L.ptr(net[r]), net.shape[2], s0, T, st))
        self.model.decoder_states(x, cond, T, sink, ratio)
        tail = _prefill_tail(x, T, self.model.pre_k)
        for h, r in zip(self._hs, rows):
            L.check(lib.vqw_ar_decode_prefill_finish(h, T, L.ptr(tail[r]) if audio else None, None if audio else L.ptr(tail[r]), st))

    def generate(self, encoding, n_steps, mode='greedy', uniforms=None, ratio=None, return_probs=False,
                 temperature=1.0, top_k=0, top_p=1.0):
        """encoding [B][Cc][Tz] (model.encode); continues from the current queue state.  temperature / top_k / top_p
        (mode 'sample' only; scalars or one value per row): see sampling_settings and vqw_ar_sampling in include/vqwave.h.
        Returns (audio [B][n] float32, indices [B][n] int32[, probs of the last step [B][Q]: the distribution sampled])."""
        _check_mode(mode)
        settings = sampling_settings(self.B, mode, temperature, top_k, top_p)
        audio = torch.empty(self.B, n_steps, device=encoding.device)
        idx, probs = self._run(encoding, n_steps, mode, uniforms, ratio or 64, audio, return_probs, settings)
        return (audio, idx, probs) if return_probs else (audio, idx)

    def _run(self, encoding, n_steps, mode, uniforms, ratio, audio, return_probs, settings=None):
        """One run of every handle over its rows; audio may be None (code mode).  settings: sampling_settings' per-row list,
        or None (every row at its defaults).  Returns (indices, probs of the last step)."""
        _check_encoding(encoding, self.B, self.model.Cc)
        L.require_cuda(encoding, uniforms)
        B, _, Tz = encoding.shape
        dev = encoding.device
        idx = torch.empty(B, n_steps, dtype=torch.int32, device=dev)
        probs = torch.empty(B, self.model.Q, device=dev) if return_probs else None
        uniforms = _uniforms_of(uniforms, mode, B, n_steps, dev, 'n_steps')
        rows = _row_slices(tuple(self._parts))
        per = [_sampling_rows(settings and settings[r]) for r in rows]     # each handle its slice of the rows

        def part(t, i):
            return None if t is None else L.ptr(t[rows[i]])

        def parts(t, wave):
            return None if t is None else (C.c_void_p * len(wave))(*[t[rows[i]].data_ptr() for i in wave])
        lib, m = L.lib(), 0 if mode == 'greedy' else 1
        for wave in self._waves:                 # one launch per wave; the waves follow each other
            if lib.vqw_ar_decode_workgroups(self._hs[wave[0]]) > 0:
                hs = (C.c_void_p * len(wave))(*[self._hs[i].value for i in wave])
                sp = None
                if settings is not None:
                    sp = (C.POINTER(L.ArSampling) * len(wave))(*[C.cast(per[i], C.POINTER(L.ArSampling)) for i in wave])
                L.check(lib.vqw_ar_decode_run_group_sampled_async(
                    hs, len(wave), parts(encoding, wave), Tz, ratio, n_steps, m, parts(uniforms, wave), sp, parts(audio, wave),
                    parts(idx, wave), parts(probs, wave), L.stream()))
            else:                                # launch-per-phase path: one handle
                i = wave[0]
                L.check(lib.vqw_ar_decode_run_sampled_async(
                    self._hs[i], part(encoding, i), Tz, ratio, n_steps, m, part(uniforms, i), per[i], part(audio, i),
                    part(idx, i), part(probs, i), L.stream()))
            for i in wave:
                L.check(lib.vqw_ar_decode_wait(self._hs[i]))
        return idx, probs

    def close(self):
        for h in getattr(self, '_hs', []):
            L.lib().vqw_ar_decode_destroy(h)
        self._hs = []


class PriorGenerator(FastGenerator):
    """Samples VQ codes from a prior.LatentPrior on the persistent generator's code-input mode (vqw_ar_prior_create): the
    history holds past codes, the preprocess gathers rows of W_pre[j][code], the sampled index is the next input.  Same
    layout policy as FastGenerator; uses the prior's LIVE variables at construction (prior.use_ema_weights() first for
    the EMA shadows).  The launch-per-phase generator (VQW_AR_PERSISTENT=0) has no code input."""

    def __init__(self, prior, batch):
        import os
        if os.environ.get('VQW_AR_PERSISTENT', '1').startswith('0'):
            raise NotImplementedError('prior sampling runs on the persistent generator only: the launch-per-phase path '
                                      '(VQW_AR_PERSISTENT=0) has no code-input mode')
        self._t = 0
        super().__init__(prior, batch)

    def _create(self, h, w, rows, cpb):
        L.check(L.lib().vqw_ar_prior_create(C.byref(h), C.byref(w), rows, cpb, self.model.Q))

    def reset(self):
        """Empty history ("no code yet": a zero one-hot, not code 0); the next sample is step 0."""
        super().reset()
        self._t = 0

    def prefill(self, codes, spk):
        """Leave every row in the state it would have after reset() and T = codes.shape[1] steps teacher-forced on its codes
        (the input of step t is c[t-1], no code at t = 0): the next sample() continues at step T.  codes int32 [B][T] in [0, k)
        on the GPU, spk int64 [B] (the speakers the later sample calls use).  T = 0 is reset()."""
        T = _check_codes(codes, spk, self.B, self.model.Q)
        cond = self.model.speaker_condition(spk.contiguous(), max(1, -(-T // PRIOR_RATIO)))
        self._prefill(codes.contiguous(), cond, T, PRIOR_RATIO, audio=False)
        self._t = T

    def sample(self, n_frames, spk, mode='greedy', uniforms=None, return_probs=False, temperature=1.0, top_k=0, top_p=1.0):
        """n_frames codes per row, continuing from the current state.  spk int64 [B] on the GPU.  mode 'greedy' (argmax) or
        'sample' (searchsorted(cumsum(p), u) with uniforms [B][n_frames], drawn here when None; u above the cdf's last
        value gives the last code), tempered / truncated by temperature, top_k, top_p as in FastGenerator.generate.
        Returns codes int32 [B][n_frames][, probabilities of the last step [B][k]: the distribution sampled]."""
        _check_mode(mode)
        settings = sampling_settings(self.B, mode, temperature, top_k, top_p)
        _check_speakers(spk, self.B)
        Tz = -(-(self._t + n_frames) // PRIOR_RATIO)
        cond = self.model.speaker_condition(spk.contiguous(), Tz)
        idx, probs = self._run(cond, n_frames, mode, uniforms, PRIOR_RATIO, None, return_probs, settings)
        self._t += n_frames
        return (idx, probs) if return_probs else idx
