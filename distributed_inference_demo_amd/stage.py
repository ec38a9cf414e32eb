"""ctypes binding of libbloomstage.so + the host-side mirror of the reference's stage interface.

Reference interface (Java side `Communication.java:1153-1182`, C++ side `native-lib.cpp`):

    long   createSession(String modelPath)                                   native-lib.cpp:671-678
    void   releaseSession(long session)                                      native-lib.cpp:1290-1303
    Object[] runInferenceMasterResidual(long, int[] ids, int[] seq, int[][] res)   :942-1034
    Object[] runInferenceWorkerResidual(long, byte[] seq, ArrayList<byte[]> res, int[], int[][])  :1036-1194
    byte[] runInferenceWorkerResidualLastGeneration(long, byte[] seq, ArrayList<byte[]> res, int k, float temp)  :1368-1443
    byte[] runInferenceWorkerResidualLastClassification(long, byte[] seq, ArrayList<byte[]> res)  :1305-1366
    int    binaryClassify(byte[])                                            :128-160
    int    deserializeInt(byte[])                                            :1445-1471

`create_session`, `release_session`, `run_inference_master_residual`,
`run_inference_worker_residual`, `run_inference_worker_residual_last_generation`,
`run_inference_worker_residual_last_classification`, `binary_classify` and `deserialize_int` below keep those names, argument meanings and wire formats (activations as
the utils.cpp tensor-vector bytes, the tail's token as 4 little-endian bytes) so the
reference's driver loop ports over unchanged.  They run the stage with host I/O.  The fast
path is `Stage.forward()` on device buffers (what the RCCL pipeline uses).

Behavioural differences, all deliberate (DESIGN.md "Boundary"): errors raise `BloomStageError`
with the library's message instead of C++ exceptions crossing JNI; the header stage feeds the
whole new-token slice and keeps a KV cache (the reference feeds only the last token with no
cache, Communication.java:322-326, so it ignores context); the tail picks the greedy argmax
(k == 1) or a seeded top-k sample (k > 1) rather than an unseeded one (decoding.cpp:61-63).
"""
import ctypes
import os
import struct

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "lib", "libbloomstage.so")

BS_DT_FLOAT = 1
BS_DT_BFLOAT16 = 16
BS_WEIGHTS_SYNTHETIC = 0
BS_WEIGHTS_HOST = 1
BS_STEP_HOST_IO = 1
BS_STEP_LOGITS = 2
BS_STEP_VERIFY = 4        # bs_step.flags: short verify pass (2 <= seq <= 8), greedy ids at every position
BS_STEP_VERIFY_DRAW = 8   # bs_step.flags, with BS_STEP_VERIFY: the row sampler's draw at every position
BS_NOTE_GENERATED = 16    # bs_note_tokens flags: the noted tokens also count as generated
BS_ROW_BIAS_MAX = 64
BS_GUIDE_MAX = 16         # guides a stage holds at a time
BS_GUIDE_SLICE = 4096     # vocabulary entries one block of the guide apply kernel owns
BS_FLAG_INT8_WEIGHTS = 1  # bs_stage_desc.flags: weight-only int8 block matrices
BS_FLAG_CLASSIFIER = 2    # bs_stage_desc.flags: sequence-classification tail (score head, class ids out)
BS_FLAG_INT8_KV = 4       # bs_stage_desc.flags: int8 KV cache, one fp32 scale per (position, head) vector
BS_FLAG_MXFP4_WEIGHTS = 8  # bs_stage_desc.flags: weight-only MXFP4 block matrices (E2M1 codes + E8M0 block scales)

DTYPES = {
    1: np.float32, 2: np.uint8, 3: np.int8, 4: np.uint16, 5: np.int16, 6: np.int32, 7: np.int64,
    9: np.bool_, 11: np.float64, 12: np.uint32, 13: np.uint64,
}
NP_TO_DT = {np.dtype(v): k for k, v in DTYPES.items()}


class BloomStageError(RuntimeError):
    pass


class StageDesc(ctypes.Structure):
    _fields_ = [
        ("hidden", ctypes.c_int32), ("n_head", ctypes.c_int32), ("n_layer", ctypes.c_int32),
        ("vocab", ctypes.c_int32), ("ln_eps", ctypes.c_float),
        ("layer_begin", ctypes.c_int32), ("layer_end", ctypes.c_int32),
        ("is_first", ctypes.c_int32), ("is_last", ctypes.c_int32),
        ("dtype", ctypes.c_int32), ("device", ctypes.c_int32),
        ("max_batch", ctypes.c_int32), ("max_ctx", ctypes.c_int32), ("max_tokens", ctypes.c_int32),
        ("weight_source", ctypes.c_int32), ("seed", ctypes.c_uint64),
        ("host_weights", ctypes.c_void_p), ("host_weight_count", ctypes.c_uint64),
        ("head_vocab_begin", ctypes.c_int32), ("head_vocab_end", ctypes.c_int32),
        ("flags", ctypes.c_int32), ("n_labels", ctypes.c_int32),
    ]


class Step(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int32), ("seq", ctypes.c_int32), ("slot", ctypes.c_int32),
                ("past_len", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("past_lens", ctypes.POINTER(ctypes.c_int32))]


class RowSampler(ctypes.Structure):
    """bs_row_sampler: the sampler state of one KV row."""
    _fields_ = [("top_k", ctypes.c_int32), ("top_p", ctypes.c_float), ("temperature", ctypes.c_float),
                ("seed", ctypes.c_uint64)]


class RowProcessor(ctypes.Structure):
    """bs_row_processor: the logit processor parameters of one KV row."""
    _fields_ = [("repetition_penalty", ctypes.c_float), ("no_repeat_ngram", ctypes.c_int32),
                ("min_new_tokens", ctypes.c_int32), ("eos_id", ctypes.c_int32), ("n_bias", ctypes.c_int32),
                ("bias_ids", ctypes.c_int32 * BS_ROW_BIAS_MAX), ("bias_values", ctypes.c_float * BS_ROW_BIAS_MAX)]


class GuideDesc(ctypes.Structure):
    """bs_guide_desc: a token automaton in CSR form (host arrays)."""
    _fields_ = [("n_states", ctypes.c_int32), ("start", ctypes.c_int32),
                ("row_ptr", ctypes.POINTER(ctypes.c_int32)), ("edge_token", ctypes.POINTER(ctypes.c_int32)),
                ("edge_next", ctypes.POINTER(ctypes.c_int32)), ("default_next", ctypes.POINTER(ctypes.c_int32))]


class RowDraw(ctypes.Structure):
    """bs_row_draw: read-out of a row's last draw."""
    _fields_ = [("threshold", ctypes.c_float), ("n_nucleus", ctypes.c_int32), ("n_candidates", ctypes.c_int32),
                ("u24", ctypes.c_uint32), ("mass_nucleus", ctypes.c_uint64), ("mass_candidates", ctypes.c_uint64),
                ("token", ctypes.c_int32), ("position", ctypes.c_int32)]


class TensorView(ctypes.Structure):
    _fields_ = [("dtype", ctypes.c_int32), ("ndim", ctypes.c_int32), ("dims", ctypes.c_int64 * 8),
                ("data", ctypes.c_void_p)]


EXPORTS = [
    "bs_init_stage", "bs_forward", "bs_reset_kv", "bs_read_kv", "bs_release", "bs_last_error", "bs_stage_info",
    "bs_stage_weight_count", "bs_abi_version", "bs_profile_enable", "bs_profile_read",
    "bs_codec_serialize", "bs_codec_deserialize", "bs_dtype_size", "bs_serialize_int", "bs_deserialize_int",
    "bs_prompt_ids", "bs_read_weights", "bs_head_norm", "bs_head_slice", "bs_stream_delay", "bs_set_sampling",
    "bs_build_id", "bs_hbm_probe", "bs_mfma_probe", "bs_init_stage_file", "bs_weights_file_probe",
    "bs_set_graphs", "bs_binary_classify", "bs_set_head_screen", "bs_read_head_screen",
    "bs_forward_score", "bs_set_row_sampler", "bs_sample_logits", "bs_read_row_draw",
    "bs_read_verify_draw", "bs_fork_kv", "bs_copy_kv", "bs_forward_topk",
    "bs_set_row_processor", "bs_note_tokens", "bs_process_logits", "bs_read_row_tokens",
    "bs_load_guide", "bs_unload_guide", "bs_set_row_guide", "bs_advance_row_guide", "bs_guide_logits",
    "bs_read_row_guide",
]

_LIB = None


def lib():
    """Load the HIP library.  There is no CPU fallback: a missing library is an error.

    A process that also uses PyTorch must import torch before the first call: torch ships its own
    libamdhip64.so.7, and the copy loaded first serves the whole process (torch fails to find the
    device on the system ROCm copy)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise BloomStageError(f"{LIB_PATH} not built: run `python -m distributed_inference_demo_amd.build`")
        L = ctypes.CDLL(LIB_PATH)
        vp, i32 = ctypes.c_void_p, ctypes.c_int32
        L.bs_build_id.restype = ctypes.c_char_p
        want, got = source_build_id(), L.bs_build_id().decode()
        if want is not None and got != want:
            raise BloomStageError(f"{LIB_PATH} was built from other sources (stamp {got[:12]}, sources {want[:12]}): "
                                  "rebuild with `python -m distributed_inference_demo_amd.build`")
        L.bs_init_stage.argtypes = [ctypes.POINTER(StageDesc), ctypes.POINTER(vp)]
        L.bs_init_stage_file.argtypes = [ctypes.POINTER(StageDesc), ctypes.c_char_p, ctypes.POINTER(vp)]
        L.bs_weights_file_probe.argtypes = [ctypes.c_char_p] + [ctypes.POINTER(i32)] * 3
        L.bs_forward.argtypes = [vp, ctypes.POINTER(Step), vp, vp, vp, vp]
        L.bs_forward_score.argtypes = [vp, ctypes.POINTER(Step), vp, vp, vp, vp, vp]
        L.bs_reset_kv.argtypes = [vp, i32]
        L.bs_read_kv.argtypes = [vp, i32, i32, i32, i32, vp]
        L.bs_fork_kv.argtypes = [vp, i32, i32, i32, i32, vp]
        L.bs_copy_kv.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32), i32, i32, vp]
        L.bs_forward_topk.argtypes = [vp, ctypes.POINTER(Step), vp, i32, vp, vp, vp, vp, vp]
        L.bs_release.argtypes = [vp]
        L.bs_release.restype = None
        L.bs_last_error.restype = ctypes.c_char_p
        L.bs_stage_info.argtypes = [vp, ctypes.POINTER(StageDesc)] + [ctypes.POINTER(ctypes.c_uint64)] * 3
        L.bs_stage_weight_count.argtypes = [ctypes.POINTER(StageDesc)]
        L.bs_stage_weight_count.restype = ctypes.c_uint64
        L.bs_profile_enable.argtypes = [vp, i32]
        L.bs_profile_read.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64),
                                      ctypes.POINTER(ctypes.c_double)]
        L.bs_stream_delay.argtypes = [vp, i32]
        L.bs_codec_serialize.argtypes = [ctypes.POINTER(TensorView), i32, vp, ctypes.c_uint64]
        L.bs_codec_serialize.restype = ctypes.c_int64
        L.bs_codec_deserialize.argtypes = [vp, ctypes.c_uint64, ctypes.POINTER(TensorView), i32, ctypes.POINTER(i32)]
        L.bs_dtype_size.argtypes = [i32]
        L.bs_dtype_size.restype = ctypes.c_int64
        L.bs_serialize_int.argtypes = [i32, ctypes.c_char_p]
        L.bs_serialize_int.restype = None
        L.bs_deserialize_int.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.POINTER(i32)]
        L.bs_binary_classify.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.POINTER(i32)]
        L.bs_prompt_ids.argtypes = [ctypes.c_uint64, i32, i32, vp]
        L.bs_read_weights.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint64, vp]
        L.bs_head_norm.argtypes = [vp, vp, i32, i32, vp, vp]
        L.bs_head_slice.argtypes = [vp, vp, i32, vp, vp, vp, vp]
        L.bs_set_sampling.argtypes = [vp, i32, ctypes.c_float, ctypes.c_uint64]
        L.bs_set_row_sampler.argtypes = [vp, i32, i32, ctypes.POINTER(RowSampler), vp]
        L.bs_sample_logits.argtypes = [vp, i32, i32, ctypes.POINTER(i32), vp, i32, vp, i32, vp]
        L.bs_read_row_draw.argtypes = [vp, i32, ctypes.POINTER(RowDraw)]
        L.bs_read_verify_draw.argtypes = [vp, i32, i32, ctypes.POINTER(RowDraw)]
        L.bs_set_row_processor.argtypes = [vp, i32, i32, ctypes.POINTER(RowProcessor), vp]
        L.bs_note_tokens.argtypes = [vp, i32, vp, i32, i32, vp]
        L.bs_process_logits.argtypes = [vp, i32, i32, vp, i32, i32, vp]
        L.bs_read_row_tokens.argtypes = [vp, i32, vp] + [ctypes.POINTER(i32)] * 3
        L.bs_load_guide.argtypes = [vp, ctypes.POINTER(GuideDesc), ctypes.POINTER(i32)]
        L.bs_unload_guide.argtypes = [vp, i32]
        L.bs_set_row_guide.argtypes = [vp, i32, i32, i32, vp, vp]
        L.bs_advance_row_guide.argtypes = [vp, i32, vp, i32, i32, vp]
        L.bs_guide_logits.argtypes = [vp, i32, i32, vp, i32, i32, vp]
        L.bs_read_row_guide.argtypes = [vp, i32] + [ctypes.POINTER(i32)] * 4
        L.bs_set_graphs.argtypes = [vp, i32]
        L.bs_set_head_screen.argtypes = [vp, i32]
        L.bs_read_head_screen.argtypes = [vp, i32, vp, vp, vp, ctypes.POINTER(i32)]
        L.bs_hbm_probe.argtypes = [i32, ctypes.c_uint64, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
        L.bs_mfma_probe.argtypes = [i32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
        _LIB = L
    return _LIB


def source_build_id():
    """SHA-256 of the library sources beside this file (the stamp build.py compiles into
    bs_build_id); None when the sources are not present (an installed library)."""
    from .build import source_hash
    try:
        return source_hash()
    except FileNotFoundError:
        return None


def _check(rc):
    if rc != 0:
        raise BloomStageError(f"bloomstage error {rc}: {lib().bs_last_error().decode(errors='replace')}")


def _ptr(x):
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    if hasattr(x, "data_ptr"):  # torch tensor
        return x.data_ptr()
    raise TypeError(f"cannot take a pointer of {type(x)}")


class Stage:
    """One pipeline stage (contiguous layer range) resident on one GPU."""

    def __init__(self, hidden, n_head, n_layer, vocab, layer_begin, layer_end, *, dtype="bf16", device=0,
                 max_batch=1, max_ctx=2048, max_tokens=0, seed=0, eps=1e-5, host_weights=None,
                 is_first=None, is_last=None, head_slice=None, int8_weights=False, weights_file=None, n_labels=0,
                 kv_int8=False, mxfp4_weights=False):
        """weights_file: a safetensors checkpoint (or its sharded *.index.json) of HF BLOOM tensors;
        the stage maps it and loads only its own layer range (bs_init_stage_file).
        n_labels > 0: a sequence-classification tail (BS_FLAG_CLASSIFIER, last stage): forwards return class ids
        and logits [batch][n_labels] instead of tokens and vocabulary logits.
        kv_int8: the KV cache holds int8 codes + one fp32 scale per (position, head) vector (BS_FLAG_INT8_KV, bf16
        stages); read_kv returns the dequantised values.
        mxfp4_weights: the four block matrices are held as OCP MXFP4 (BS_FLAG_MXFP4_WEIGHTS, bf16 stages, opt-in:
        round-to-nearest 4-bit weights are lossy); read_weights returns the dequantised values, which are exact in
        bf16, so a plain bf16 stage given them as host_weights is the same model."""
        if weights_file is not None and host_weights is not None:
            raise ValueError("pass host_weights or weights_file, not both")
        d = StageDesc()
        d.hidden, d.n_head, d.n_layer, d.vocab, d.ln_eps = hidden, n_head, n_layer, vocab, eps
        d.layer_begin, d.layer_end = layer_begin, layer_end
        d.is_first = int(layer_begin == 0 if is_first is None else is_first)
        d.is_last = int(layer_end == n_layer if is_last is None else is_last)
        d.dtype = BS_DT_BFLOAT16 if dtype in ("bf16", BS_DT_BFLOAT16) else BS_DT_FLOAT
        d.device, d.max_batch, d.max_ctx, d.max_tokens = device, max_batch, max_ctx, max_tokens
        d.seed = seed
        d.flags = BS_FLAG_INT8_WEIGHTS if int8_weights else 0  # bloom*-int8 variants (server.py:796-799)
        if mxfp4_weights:
            d.flags |= BS_FLAG_MXFP4_WEIGHTS
        if kv_int8:
            d.flags |= BS_FLAG_INT8_KV
        if n_labels:
            d.flags |= BS_FLAG_CLASSIFIER
            d.n_labels = n_labels
        if head_slice is not None:
            d.head_vocab_begin, d.head_vocab_end = head_slice
        self._weights_ref = None
        if host_weights is not None:
            w = np.ascontiguousarray(host_weights, dtype=np.float32).reshape(-1)
            self._weights_ref = w
            d.weight_source = BS_WEIGHTS_HOST
            d.host_weights = w.ctypes.data
            d.host_weight_count = w.size
        else:
            d.weight_source = BS_WEIGHTS_SYNTHETIC
        self.desc = d
        self.hidden, self.vocab = hidden, vocab
        self.n_labels = n_labels
        self.kv_int8 = bool(kv_int8)
        self.n_out = n_labels if n_labels else vocab  # logits per row of the last stage
        self.is_first, self.is_last = bool(d.is_first), bool(d.is_last)
        self.max_batch, self.max_ctx = max_batch, max_ctx
        h = ctypes.c_void_p()
        if weights_file is not None:
            _check(lib().bs_init_stage_file(ctypes.byref(d), os.fsencode(weights_file), ctypes.byref(h)))
        else:
            _check(lib().bs_init_stage(ctypes.byref(d), ctypes.byref(h)))
        self._h = h
        self._weights_ref = None  # uploaded; host copy no longer needed
        self._steps = {}  # decode fast path: re-used Step structs
        self._fwd = lib().bs_forward
        self.past = [0] * max_batch  # host mirror of cached positions per KV row

    def _step(self, batch, seq, slot, past_len, flags):
        """Step struct; past_len is an int (every row) or a sequence of per-row positions.
        Returns (step, per-row pasts)."""
        if past_len is None:
            past_len = self.past[slot:slot + batch] if 0 <= slot and slot + batch <= len(self.past) else 0
        if isinstance(past_len, int):  # the decode fast path: a Step per (batch, seq, slot, flags), re-used
            key = (batch, seq, slot, flags)
            st = self._steps.get(key)
            if st is None:
                st = self._steps[key] = Step(batch, seq, slot, past_len, flags, None)
            st.past_len = past_len
            return st, None
        if np.ndim(past_len) == 0:
            pasts = [int(past_len)] * batch
            st = Step(batch, seq, slot, int(past_len), flags, None)
        else:
            pasts = [int(p) for p in past_len]
            if len(pasts) != batch:
                raise BloomStageError(f"{len(pasts)} past lengths for {batch} rows")
            arr = (ctypes.c_int32 * batch)(*pasts)
            st = Step(batch, seq, slot, pasts[0], flags, arr)
            st._keep = arr
        return st, pasts

    # ---- fast path (device pointers, stream ordered)
    @staticmethod
    def _verify_flags(verify, draw):
        if draw and not verify:
            raise ValueError("draw=True needs verify=True (BS_STEP_VERIFY_DRAW is a verify pass's flag)")
        return (BS_STEP_VERIFY if verify else 0) | (BS_STEP_VERIFY_DRAW if draw else 0)

    def forward(self, inp, out, batch, seq, slot=0, past_len=None, logits=None, stream=None, verify=False,
                draw=False):
        """past_len: positions already cached, one int for every row or one per row (None: the
        host mirror of each row's position).
        verify: a BS_STEP_VERIFY pass (2 <= seq <= 8, batch * seq <= 32): the last stage writes int32 ids
        [batch][seq], the greedy token of every position (logits: fp32 [batch][seq][vocab]); on device buffers it
        replays a captured graph like a decode step.
        draw (with verify): BS_STEP_VERIFY_DRAW -- rows that hold sampler state (set_row_sampler) get their own draw
        at every position instead of the greedy id; a non-last stage ignores it."""
        flags = (BS_STEP_LOGITS if logits is not None else 0) | self._verify_flags(verify, draw)
        st, pasts = self._step(batch, seq, slot, past_len, flags)
        _check(self._fwd(self._h, ctypes.byref(st), _ptr(inp), _ptr(out), _ptr(logits), stream))
        if pasts is None:
            self.past[slot:slot + batch] = [st.past_len + seq] * batch
        else:
            for i, r in enumerate(range(slot, slot + batch)):
                self.past[r] = pasts[i] + seq
        return out

    def _advance(self, st, pasts, batch, seq, slot):
        if pasts is None:
            self.past[slot:slot + batch] = [st.past_len + seq] * batch
        else:
            for i, r in enumerate(range(slot, slot + batch)):
                self.past[r] = pasts[i] + seq

    # ---- teacher-forced scoring (bs_forward_score; last stage of a bf16 generation model)
    def score(self, inp, targets, top_ids, scores, batch, seq, slot=0, past_len=None, stream=None):
        """Log-probabilities and greedy ids at every position, on device pointers (stream ordered).
        inp: forward()'s input; targets: int32 [batch][seq] (-1 = none) or None; top_ids: int32 [batch][seq] or
        None; scores: fp32 [batch][seq][3] = (log p(target), log p(top id), logsumexp) or None.  Appends seq
        positions to the KV rows like forward(), so a long text scores in chunks with past_len."""
        st, pasts = self._step(batch, seq, slot, past_len, 0)
        _check(lib().bs_forward_score(self._h, ctypes.byref(st), _ptr(inp), _ptr(targets), _ptr(top_ids),
                                      _ptr(scores), stream))
        self._advance(st, pasts, batch, seq, slot)
        return top_ids, scores

    def score_host(self, x, targets, batch, seq, slot=0, past_len=None):
        """score() with numpy in and out: returns (top_ids int32 [batch][seq], scores fp32 [batch][seq][3])."""
        if self.is_first:
            x = np.ascontiguousarray(x, dtype=np.int32).reshape(batch, seq)
        else:
            x = np.ascontiguousarray(x, dtype=np.float32).reshape(batch, seq, self.hidden)
        if targets is not None:
            targets = np.ascontiguousarray(targets, dtype=np.int32).reshape(batch, seq)
        top = np.empty((batch, seq), np.int32)
        scores = np.empty((batch, seq, 3), np.float32)
        st, pasts = self._step(batch, seq, slot, past_len, BS_STEP_HOST_IO)
        _check(lib().bs_forward_score(self._h, ctypes.byref(st), x.ctypes.data, _ptr(targets), top.ctypes.data,
                                      scores.ctypes.data, None))
        self._advance(st, pasts, batch, seq, slot)
        return top, scores

    # ---- top-k log-prob pass (bs_forward_topk; last stage of a generation model)
    def forward_topk(self, inp, ids, logprobs, batch, seq, k, slot=0, past_len=None, lse=None, logits=None,
                     stream=None):
        """The k <= 16 best tokens of each row's last position on device pointers (stream ordered): ids int32
        [batch][k] (larger logit first, the lower index first on ties), logprobs fp32 [batch][k], and optionally lse
        fp32 [batch] and logits fp32 [batch][vocab].  Appends seq positions to the KV rows like forward(); seq == 1
        replays a captured graph."""
        st, pasts = self._step(batch, seq, slot, past_len, 0)
        _check(lib().bs_forward_topk(self._h, ctypes.byref(st), _ptr(inp), int(k), _ptr(ids), _ptr(logprobs),
                                     _ptr(lse), _ptr(logits), stream))
        self._advance(st, pasts, batch, seq, slot)
        return ids, logprobs

    def forward_topk_host(self, x, batch, seq, k, slot=0, past_len=None, want_logits=False):
        """forward_topk() with numpy in and out: returns (ids int32 [batch][k], logprobs fp32 [batch][k], lse fp32
        [batch]) and, with want_logits, the logits fp32 [batch][vocab] as a fourth item."""
        if self.is_first:
            x = np.ascontiguousarray(x, dtype=np.int32).reshape(batch, seq)
        else:
            x = np.ascontiguousarray(x, dtype=np.float32).reshape(batch, seq, self.hidden)
        ids = np.empty((batch, k), np.int32)
        lp = np.empty((batch, k), np.float32)
        lse = np.empty(batch, np.float32)
        logits = np.empty((batch, self.vocab), np.float32) if want_logits else None
        st, pasts = self._step(batch, seq, slot, past_len, BS_STEP_HOST_IO)
        _check(lib().bs_forward_topk(self._h, ctypes.byref(st), x.ctypes.data, int(k), ids.ctypes.data, lp.ctypes.data,
                                     lse.ctypes.data, _ptr(logits), None))
        self._advance(st, pasts, batch, seq, slot)
        return (ids, lp, lse, logits) if want_logits else (ids, lp, lse)

    def set_sampling(self, top_k=1, temperature=1.0, seed=0):
        """Tail token pick (bs_set_sampling): greedy for top_k <= 1, else seeded top-k sampling in
        decoding.cpp:24-66's order (last stage only)."""
        _check(lib().bs_set_sampling(self._h, int(top_k), float(temperature), int(seed)))

    # ---- per-row sampling (bs_set_row_sampler; last stage of a generation model)
    def set_row_sampler(self, slot, top_k=0, top_p=1.0, temperature=1.0, seed=0, count=1, stream=None):
        """Give KV rows [slot, slot + count) a sampler state: top-k (0 = none) / top-p / temperature and the seed of
        the draws, keyed by (seed, position) only.  Every parameter is one value for all the rows or a sequence of
        `count` values.  Stream ordered; captured decode graphs stay."""
        def per_row(v):
            vs = list(v) if np.ndim(v) else [v] * count
            if len(vs) != count:
                raise BloomStageError(f"{len(vs)} sampler values for {count} rows")
            return vs
        ks, ps, ts, ss = per_row(top_k), per_row(top_p), per_row(temperature), per_row(seed)
        arr = (RowSampler * count)(*[RowSampler(int(ks[i]), float(ps[i]), float(ts[i]), int(ss[i]) & (2**64 - 1))
                                     for i in range(count)])
        _check(lib().bs_set_row_sampler(self._h, int(slot), int(count), arr, stream))

    def clear_row_sampler(self, slot=None, count=1, stream=None):
        """Back to greedy for rows [slot, slot + count), or for every row when slot is None."""
        if slot is None:
            slot, count = 0, self.max_batch
        _check(lib().bs_set_row_sampler(self._h, int(slot), int(count), None, stream))

    def sample_logits(self, logits, positions, slot=0, tokens=None, ld=None, stream=None):
        """bs_sample_logits: run the tail's row sampler on given logits for rows [slot, slot + batch) at
        `positions` (one int per row).  logits: a numpy array [batch][ld] (host I/O; returns the tokens as int32
        [batch]) or a device pointer / torch tensor with `tokens` a device buffer of batch int32 (stream ordered)."""
        pos = [int(p) for p in np.atleast_1d(positions)]
        batch = len(pos)
        parr = (ctypes.c_int32 * batch)(*pos)
        if isinstance(logits, np.ndarray):
            lg = np.ascontiguousarray(logits, dtype=np.float32).reshape(batch, -1)
            out = np.empty(batch, np.int32)
            _check(lib().bs_sample_logits(self._h, int(slot), batch, parr, lg.ctypes.data, lg.shape[1],
                                          out.ctypes.data, BS_STEP_HOST_IO, stream))
            return out
        _check(lib().bs_sample_logits(self._h, int(slot), batch, parr, _ptr(logits), int(ld or self.vocab),
                                      _ptr(tokens), 0, stream))
        return tokens

    def read_row_draw(self, slot):
        """bs_read_row_draw: {"threshold", "n_nucleus", "n_candidates", "u24", "mass_nucleus", "mass_candidates"
        (2^40 fixed point), "token", "position"} of row `slot`'s last draw.  Synchronises."""
        d = RowDraw()
        _check(lib().bs_read_row_draw(self._h, int(slot), ctypes.byref(d)))
        return {name: getattr(d, name) for name, _ in RowDraw._fields_}

    def read_verify_draw(self, slot, t):
        """bs_read_verify_draw: read_row_draw's dict for position `t` of KV row `slot` in the stage's last verify
        pass with draw=True that ran the sampler.  Synchronises."""
        d = RowDraw()
        _check(lib().bs_read_verify_draw(self._h, int(slot), int(t), ctypes.byref(d)))
        return {name: getattr(d, name) for name, _ in RowDraw._fields_}

    # ---- per-row logit processors (bs_set_row_processor; last stage of a generation model)
    @staticmethod
    def row_processor(repetition_penalty=1.0, no_repeat_ngram=0, min_new_tokens=0, eos_id=-1, bias=(), bad_tokens=()):
        """A RowProcessor from keyword values: bias = (token, value) pairs or a dict, bad_tokens = banned ids (entries
        of -inf)."""
        ent = [(int(t), float(v)) for t, v in (bias.items() if isinstance(bias, dict) else bias)]
        ent += [(int(t), float("-inf")) for t in bad_tokens]
        if len(ent) > BS_ROW_BIAS_MAX:
            raise BloomStageError(f"{len(ent)} bias / ban entries: a row holds at most {BS_ROW_BIAS_MAX}")
        p = RowProcessor(float(repetition_penalty), int(no_repeat_ngram), int(min_new_tokens), int(eos_id), len(ent))
        for i, (t, v) in enumerate(ent):
            p.bias_ids[i], p.bias_values[i] = t, v
        return p

    def set_row_processor(self, slot, params=None, count=1, stream=None, **kw):
        """Give KV rows [slot, slot + count) a logit processor state and empty their token history: `params` is one
        RowProcessor for all the rows or a sequence of `count`; without it the keywords of row_processor() make one.
        Stream ordered; captured decode graphs stay."""
        if params is None:
            params = self.row_processor(**kw)
        ps = [params] * count if isinstance(params, RowProcessor) else list(params)
        if len(ps) != count:
            raise BloomStageError(f"{len(ps)} processor states for {count} rows")
        _check(lib().bs_set_row_processor(self._h, int(slot), int(count), (RowProcessor * count)(*ps), stream))

    def clear_row_processor(self, slot=None, count=1, stream=None):
        """Drop the processor state and the token history of rows [slot, slot + count), or of every row (None)."""
        if slot is None:
            slot, count = 0, self.max_batch
        _check(lib().bs_set_row_processor(self._h, int(slot), int(count), None, stream))

    def note_tokens(self, slot, ids, n=None, generated=False, stream=None):
        """bs_note_tokens: append tokens to row `slot`'s history (its prompt).  ids: a sequence / numpy array (host,
        read before the call returns) or a device pointer / torch tensor of n int32 (read on the stream)."""
        flags = BS_NOTE_GENERATED if generated else 0
        if isinstance(ids, int) or hasattr(ids, "data_ptr"):
            n = int(ids.numel() if n is None else n) if hasattr(ids, "data_ptr") else int(n)
            _check(lib().bs_note_tokens(self._h, int(slot), _ptr(ids), n, flags, stream))
            return
        arr = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        _check(lib().bs_note_tokens(self._h, int(slot), arr.ctypes.data, arr.size, flags | BS_STEP_HOST_IO, stream))

    def process_logits(self, logits, slot=0, batch=None, ld=None, stream=None):
        """bs_process_logits: the tail's apply kernel in place on given logits for rows [slot, slot + batch).  logits: a
        numpy array [batch][ld] (host I/O; returns the processed copy) or a device pointer / torch tensor (in place)."""
        if isinstance(logits, np.ndarray):
            lg = np.array(logits, dtype=np.float32, order="C")
            lg = lg.reshape(1, -1) if lg.ndim == 1 else lg
            _check(lib().bs_process_logits(self._h, int(slot), lg.shape[0], lg.ctypes.data, lg.shape[1],
                                           BS_STEP_HOST_IO, stream))
            return lg
        _check(lib().bs_process_logits(self._h, int(slot), int(batch), _ptr(logits), int(ld or self.vocab), 0, stream))
        return logits

    def read_row_tokens(self, slot):
        """bs_read_row_tokens: {"tokens": the ordered history (int32), "generated", "distinct"} of row `slot`.
        Synchronises."""
        buf = np.empty(self.max_ctx + 1, np.int32)
        n, g, d = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        _check(lib().bs_read_row_tokens(self._h, int(slot), buf.ctypes.data, ctypes.byref(n), ctypes.byref(g),
                                        ctypes.byref(d)))
        return {"tokens": buf[:n.value].copy(), "generated": g.value, "distinct": d.value}

    # ---- guided decoding (bs_load_guide; last stage of a generation model)
    def load_guide(self, guide):
        """bs_load_guide: copy a token automaton to the device and return its id.  `guide`: anything with n_states,
        start, row_ptr, edge_token, edge_next and default_next (guide.Guide), or a dict of them.  May synchronise."""
        get = guide.__getitem__ if isinstance(guide, dict) else lambda k: getattr(guide, k)
        arrs = [np.ascontiguousarray(get(k), dtype=np.int32).reshape(-1)
                for k in ("row_ptr", "edge_token", "edge_next", "default_next")]
        ip = ctypes.POINTER(ctypes.c_int32)
        d = GuideDesc(int(get("n_states")), int(get("start")), *[a.ctypes.data_as(ip) for a in arrs])
        gid = ctypes.c_int32(-1)
        _check(lib().bs_load_guide(self._h, ctypes.byref(d), ctypes.byref(gid)))
        return gid.value

    def unload_guide(self, guide_id):
        """bs_unload_guide: free a guide no row references.  Synchronises."""
        _check(lib().bs_unload_guide(self._h, int(guide_id)))

    def set_row_guide(self, slot, guide_id, states=None, count=1, stream=None):
        """bs_set_row_guide: give KV rows [slot, slot + count) the guide and a state each (`states`: one int for all
        the rows, a sequence of `count`, or None for the guide's start state) and zero their counters.  Stream ordered;
        captured decode graphs stay."""
        st = None
        if states is not None:
            st = np.ascontiguousarray([states] * count if np.isscalar(states) else states, dtype=np.int32).reshape(-1)
            if st.size != count:
                raise BloomStageError(f"{st.size} guide states for {count} rows")
        _check(lib().bs_set_row_guide(self._h, int(slot), int(count), int(guide_id),
                                      None if st is None else st.ctypes.data, stream))

    def clear_row_guide(self, slot=None, count=1, stream=None):
        """Drop the guide state of rows [slot, slot + count), or of every row (None)."""
        if slot is None:
            slot, count = 0, self.max_batch
        _check(lib().bs_set_row_guide(self._h, int(slot), int(count), -1, None, stream))

    def advance_row_guide(self, slot, ids, n=None, stream=None):
        """bs_advance_row_guide: walk tokens through row `slot`'s guide state.  ids: a sequence / numpy array (host, read
        before the call returns) or a device pointer / torch tensor of n int32 (read on the stream)."""
        if isinstance(ids, int) or hasattr(ids, "data_ptr"):
            n = int(ids.numel() if n is None else n) if hasattr(ids, "data_ptr") else int(n)
            _check(lib().bs_advance_row_guide(self._h, int(slot), _ptr(ids), n, 0, stream))
            return
        arr = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        _check(lib().bs_advance_row_guide(self._h, int(slot), arr.ctypes.data, arr.size, BS_STEP_HOST_IO, stream))

    def guide_logits(self, logits, slot=0, batch=None, ld=None, stream=None):
        """bs_guide_logits: the tail's guide apply kernel in place on given logits for rows [slot, slot + batch).
        logits: a numpy array [batch][ld] (host I/O; returns the masked copy) or a device pointer / torch tensor."""
        if isinstance(logits, np.ndarray):
            lg = np.array(logits, dtype=np.float32, order="C")
            lg = lg.reshape(1, -1) if lg.ndim == 1 else lg
            _check(lib().bs_guide_logits(self._h, int(slot), lg.shape[0], lg.ctypes.data, lg.shape[1],
                                         BS_STEP_HOST_IO, stream))
            return lg
        _check(lib().bs_guide_logits(self._h, int(slot), int(batch), _ptr(logits), int(ld or self.vocab), 0, stream))
        return logits

    def read_row_guide(self, slot):
        """bs_read_row_guide: {"guide", "state", "n_steps", "n_rejected"} of row `slot` (guide -1: none).
        Synchronises."""
        v = [ctypes.c_int32() for _ in range(4)]
        _check(lib().bs_read_row_guide(self._h, int(slot), *[ctypes.byref(x) for x in v]))
        return dict(zip(("guide", "state", "n_steps", "n_rejected"), (x.value for x in v)))

    def set_graphs(self, on=True):
        """bs_set_graphs: replay captured decode graphs (default) or launch every step eagerly."""
        _check(lib().bs_set_graphs(self._h, 1 if on else 0))

    def set_head_screen(self, on=True):
        """bs_set_head_screen: greedy steps of <= 2 rows screen the lm_head on its int8 shadow copy and re-score
        the few candidate tiles exactly (default where the copy exists), or always run the full head."""
        _check(lib().bs_set_head_screen(self._h, 1 if on else 0))

    def read_head_screen(self, row=0):
        """bs_read_head_screen for row `row` of the last forward: None when its tail took the full head, else
        {"hi", "lo": fp32 [vocab/16] bounds of each 16-row tile's largest logit, "lstar": the largest lo,
        "tiles": the candidate tiles, sorted}."""
        nt = self.vocab // 16
        hilo = np.empty((nt, 2), np.float32)
        lstar = np.empty(1, np.float32)
        tiles = np.empty(nt, np.int32)
        n = ctypes.c_int32()
        _check(lib().bs_read_head_screen(self._h, row, hilo.ctypes.data, lstar.ctypes.data, tiles.ctypes.data,
                                         ctypes.byref(n)))
        if n.value < 0:
            return None
        return {"hi": hilo[:, 0].copy(), "lo": hilo[:, 1].copy(), "lstar": float(lstar[0]),
                "tiles": np.sort(tiles[:n.value])}

    # ---- vocabulary-parallel head (device pointers, stream ordered)
    def head_norm(self, hidden, batch, seq, xn, stream=None):
        """ln_f of each row's last position -> xn [batch][hidden] (stage activation dtype)."""
        _check(lib().bs_head_norm(self._h, _ptr(hidden), batch, seq, _ptr(xn), stream))

    def head_slice(self, xn, batch, keys_in=None, keys_out=None, tokens=None, stream=None):
        """Argmax keys of this stage's vocabulary slice, merged with keys_in (uint64 [batch])."""
        _check(lib().bs_head_slice(self._h, _ptr(xn), batch, _ptr(keys_in), _ptr(keys_out), _ptr(tokens), stream))

    # ---- host I/O convenience (numpy in, numpy out)
    def forward_host(self, x, batch, seq, slot=0, past_len=None, want_logits=False, verify=False, draw=False):
        """verify: a BS_STEP_VERIFY pass; the last stage returns ids [batch][seq] (and logits [batch][seq][vocab]).
        draw (with verify): BS_STEP_VERIFY_DRAW, the ids of rows with sampler state are their draws."""
        if self.is_first:
            x = np.ascontiguousarray(x, dtype=np.int32).reshape(batch, seq)
        else:
            x = np.ascontiguousarray(x, dtype=np.float32).reshape(batch, seq, self.hidden)
        rows = (batch, seq) if verify else (batch,)
        out = np.empty(rows, np.int32) if self.is_last else np.empty((batch, seq, self.hidden), np.float32)
        logits = np.empty(rows + (self.n_out,), np.float32) if want_logits else None
        flags = BS_STEP_HOST_IO | (BS_STEP_LOGITS if want_logits else 0) | self._verify_flags(verify, draw)
        st, pasts = self._step(batch, seq, slot, past_len, flags)
        _check(lib().bs_forward(self._h, ctypes.byref(st), x.ctypes.data, out.ctypes.data,
                                logits.ctypes.data if logits is not None else None, None))
        if pasts is None:
            self.past[slot:slot + batch] = [st.past_len + seq] * batch
        else:
            for i, r in enumerate(range(slot, slot + batch)):
                self.past[r] = pasts[i] + seq
        return (out, logits) if want_logits else out

    def rollback(self, slot, pos):
        """Forget the positions of KV row `slot` at and beyond `pos` (speculative decoding: the rejected drafts).
        Only the host mirror moves: positions are passed per call, and no kernel reads a cache entry at or beyond
        its row's position."""
        if not 0 <= pos <= self.past[slot]:
            raise BloomStageError(f"rollback of row {slot} to {pos}: it holds {self.past[slot]} positions")
        self.past[slot] = pos

    def reset(self, slot=-1):
        _check(lib().bs_reset_kv(self._h, slot))
        if slot < 0:
            self.past = [0] * self.max_batch
        else:
            self.past[slot] = 0

    def fork_kv(self, src, dst, npos=None, count=1, stream=None):
        """bs_fork_kv: copy cached positions [0, npos) of KV row `src` to rows [dst, dst + count), every layer of the
        stage (npos None: all the positions the host mirror holds for `src`).  Stream ordered like forward(); the
        forked rows then stand at npos.  Sampler state is per row and is not copied."""
        if npos is None:
            npos = self.past[src]
        _check(lib().bs_fork_kv(self._h, int(src), int(dst), int(count), int(npos), stream))
        self.past[dst:dst + count] = [int(npos)] * count

    def copy_kv(self, pairs, npos, stream=None):
        """bs_copy_kv: cached positions [0, npos) of row src to row dst for every (src, dst) of `pairs` (at most 32),
        every layer of the stage (fork launches, one per run of pairs with one source and consecutive destinations).
        No destination may be a source or appear twice.  Stream ordered like forward(); the destination rows then
        stand at npos."""
        pairs = [(int(a), int(b)) for a, b in pairs]
        n = len(pairs)
        src = (ctypes.c_int32 * max(n, 1))(*[a for a, _ in pairs])
        dst = (ctypes.c_int32 * max(n, 1))(*[b for _, b in pairs])
        _check(lib().bs_copy_kv(self._h, src, dst, n, int(npos), stream))
        for _, b in pairs:
            self.past[b] = int(npos)

    def read_kv(self, layer, slot, pos0, npos):
        """KV row `slot` of local layer `layer`, positions [pos0, pos0+npos): fp32 [2 (K, V)][n_head][npos][hd]."""
        nh = self.desc.n_head
        out = np.empty((2, nh, npos, self.hidden // nh), np.float32)
        _check(lib().bs_read_kv(self._h, layer, slot, pos0, npos, out.ctypes.data))
        return out

    def info(self):
        d = StageDesc()
        wb, kb, sb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().bs_stage_info(self._h, ctypes.byref(d), ctypes.byref(wb), ctypes.byref(kb), ctypes.byref(sb)))
        return {"weight_bytes": wb.value, "kv_bytes": kb.value, "workspace_bytes": sb.value}

    def read_weights(self, offset=0, count=None):
        """Weights in canonical stage order (BS_WEIGHTS_HOST layout) as fp32."""
        if count is None:
            count = lib().bs_stage_weight_count(ctypes.byref(self.desc)) - offset
        out = np.empty(count, np.float32)
        _check(lib().bs_read_weights(self._h, offset, count, out.ctypes.data))
        return out

    def profile_enable(self, kernel_class):
        _check(lib().bs_profile_enable(self._h, kernel_class))

    @staticmethod
    def stream_delay(stream, microseconds):
        """Spin the stream for `microseconds` so the host can enqueue ahead of the GPU."""
        _check(lib().bs_stream_delay(stream, microseconds))

    def profile_read(self):
        ms, n, units = ctypes.c_double(), ctypes.c_uint64(), ctypes.c_double()
        _check(lib().bs_profile_read(self._h, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(units)))
        return ms.value, n.value, units.value

    def close(self):
        if getattr(self, "_h", None):
            lib().bs_release(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def prompt_ids(seed, batch, seq, vocab):
    """Synthetic prompt ids [batch][seq] (repo generator, computed by the library)."""
    out = np.empty((batch, seq), np.int32)
    _check(lib().bs_prompt_ids(seed, batch * seq, vocab, out.ctypes.data))
    return out


def hbm_probe(device=0, nbytes=2 << 30):
    """STREAM-like (read GB/s, copy GB/s) of a device (bs_hbm_probe)."""
    r, c = ctypes.c_double(), ctypes.c_double()
    _check(lib().bs_hbm_probe(device, nbytes, ctypes.byref(r), ctypes.byref(c)))
    return r.value, c.value


def mfma_probe(device=0):
    """Measured dense bf16 MFMA TFLOP/s of a device (bs_mfma_probe): (32x32x16 chains, 16x16x32 chains)."""
    a, b = ctypes.c_double(), ctypes.c_double()
    _check(lib().bs_mfma_probe(device, ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


def probe_weights_file(path):
    """(hidden, n_layer, vocab) a checkpoint implies (bs_weights_file_probe); -1 where unknown."""
    v = [ctypes.c_int32() for _ in range(3)]
    _check(lib().bs_weights_file_probe(os.fsencode(path), *[ctypes.byref(x) for x in v]))
    return tuple(x.value for x in v)


def weight_count(**kw):
    d = StageDesc()
    for k, v in kw.items():
        setattr(d, k, v)
    return lib().bs_stage_weight_count(ctypes.byref(d))


# ---------------------------------------------------------------------------------------
# Wire codec (utils.cpp:124-368) through the C library.
# ---------------------------------------------------------------------------------------
def serialize_tensors(arrays) -> bytes:
    """SerializeTensorVectorToBytes (utils.cpp:124-264)."""
    arrays = [np.asarray(a) for a in arrays]
    arrays = [a if a.flags.c_contiguous else a.copy(order="C") for a in arrays]  # keeps 0-d shapes
    views = (TensorView * max(1, len(arrays)))()
    for i, a in enumerate(arrays):
        if a.dtype not in NP_TO_DT:
            raise BloomStageError(f"dtype {a.dtype} is not carried by the reference wire codec")
        views[i].dtype = NP_TO_DT[a.dtype]
        views[i].ndim = a.ndim
        for k, s in enumerate(a.shape):
            views[i].dims[k] = s
        views[i].data = a.ctypes.data if a.size else None
    n = lib().bs_codec_serialize(views, len(arrays), None, 0)
    if n < 0:
        raise BloomStageError(f"serialize failed ({n})")
    buf = ctypes.create_string_buffer(n)
    m = lib().bs_codec_serialize(views, len(arrays), buf, n)
    if m != n:
        raise BloomStageError(f"serialize failed ({m})")
    return buf.raw


def deserialize_tensors(data: bytes):
    """DeserializeTensorVectorFromBytes (utils.cpp:266-368); returns copies as numpy arrays."""
    n = ctypes.c_int32()
    buf = ctypes.create_string_buffer(bytes(data), len(data))
    rc = lib().bs_codec_deserialize(buf, len(data), None, 0, ctypes.byref(n))
    if rc != 0:
        raise BloomStageError(f"deserialize failed ({rc})")
    views = (TensorView * max(1, n.value))()
    _check(lib().bs_codec_deserialize(buf, len(data), views, n.value, ctypes.byref(n)))
    base = ctypes.addressof(buf)
    out = []
    for i in range(n.value):
        v = views[i]
        dt = np.dtype(DTYPES[v.dtype])
        shape = tuple(v.dims[k] for k in range(v.ndim))
        cnt = int(np.prod(shape)) if shape else 1
        off = (v.data or base) - base
        out.append(np.frombuffer(buf.raw, dtype=dt, count=cnt, offset=off).reshape(shape).copy())
    return out


def serialize_int(value: int) -> bytes:
    """SerializeInt (utils.cpp:11-15): 4 native little-endian bytes."""
    b = ctypes.create_string_buffer(4)
    lib().bs_serialize_int(value, b)
    return b.raw


def deserialize_int(data: bytes) -> int:
    """Java_..._deserializeInt (native-lib.cpp:1445-1471) / utils::DeserializeInt (utils.cpp:17-25)."""
    v = ctypes.c_int32()
    _check(lib().bs_deserialize_int(bytes(data), len(data), ctypes.byref(v)))
    return v.value


# ---------------------------------------------------------------------------------------
# JNI-mirror entry points (host I/O, one sample per session like the reference).
# ---------------------------------------------------------------------------------------
def create_session(model, layer_begin, layer_end, **kw) -> Stage:
    """createSession (native-lib.cpp:671-678): one module == one contiguous layer range of `model`
    (a BloomDims from .config) on a GPU."""
    return Stage(model.hidden, model.n_head, model.n_layer, model.vocab, layer_begin, layer_end, **kw)


def release_session(stage: Stage) -> None:
    """releaseSession (native-lib.cpp:1290-1303)."""
    stage.close()


def run_inference_master_residual(stage: Stage, input_ids, to_send_seq_indices=(0,), to_send_res_indices=()):
    """runInferenceMasterResidual (native-lib.cpp:942-1034): header stage on new token ids.
    Returns (seq_bytes, [residual_bytes...]) like the JNI Object[]{byte[], byte[][]}; this build
    forwards only the hidden state, so the residual list is empty."""
    if not stage.is_first:
        raise BloomStageError("master (header) entry called on a non-first stage")
    ids = np.asarray(input_ids, dtype=np.int32).reshape(1, -1)
    hidden = stage.forward_host(ids, 1, ids.shape[1])
    return serialize_tensors([hidden]), []


def run_inference_worker_residual(stage: Stage, seq_bytes: bytes, residuals=(), to_send_seq_indices=(0,),
                                  to_send_res_indices=()):
    """runInferenceWorkerResidual (native-lib.cpp:1036-1194): middle stage, wire bytes in/out."""
    tensors = deserialize_tensors(seq_bytes)
    x = tensors[0].astype(np.float32, copy=False)
    S = x.shape[-2]
    hidden = stage.forward_host(x, 1, S)
    return serialize_tensors([hidden]), []


def run_inference_worker_residual_last_generation(stage: Stage, seq_bytes: bytes, residuals=(), k: int = 1,
                                                  initial_temp: float = 1.0, seed: int = 0) -> bytes:
    """runInferenceWorkerResidualLastGeneration (native-lib.cpp:1368-1443): tail stage, returns the
    next token id as 4 little-endian bytes (utils::SerializeInt).  k <= 1: greedy argmax; k > 1:
    the device top-k pick of decoding::StaticDecoding (decoding.cpp:24-66, bs_set_sampling), seeded
    by `seed` and keyed by the row's position, so every step draws afresh.  Like the reference
    (decoding.cpp:51-52), initial_temp is accepted and not applied."""
    tensors = deserialize_tensors(seq_bytes)
    x = tensors[0].astype(np.float32, copy=False)
    S = x.shape[-2]
    pick = (max(1, int(k)), int(seed))
    if getattr(stage, "_pick", (1, 0)) != pick:
        stage.set_sampling(pick[0], 1.0, pick[1])
        stage._pick = pick
    tok = stage.forward_host(x, 1, S)
    return serialize_int(int(tok[0]))


def run_inference_worker_residual_last_classification(stage: Stage, seq_bytes: bytes, residuals=()) -> bytes:
    """runInferenceWorkerResidualLastClassification (native-lib.cpp:1305-1366): classifier tail stage
    (Stage(..., n_labels=...)), returns the class of the sample -- the first index of the largest score logit,
    inference::binary_classify (inference.cpp:57-69) -- as 4 little-endian bytes (utils::SerializeInt)."""
    if not stage.n_labels:
        raise BloomStageError("classification entry called on a stage without a classifier head")
    x = deserialize_tensors(seq_bytes)[0].astype(np.float32, copy=False)
    cls = stage.forward_host(x, 1, x.shape[-2])
    return serialize_int(int(cls[0]))


def binary_classify(data: bytes) -> int:
    """binaryClassify (native-lib.cpp:128-160): the first tensor of a wire buffer holds logits; the class is the
    first index of the larger of its first two floats (bs_binary_classify)."""
    v = ctypes.c_int32()
    _check(lib().bs_binary_classify(bytes(data), len(data), ctypes.byref(v)))
    return v.value


def unpack_int_be(data: bytes) -> int:
    """Java-side big-endian int codec (Utils.java:107-125), for the sample-id frames."""
    return struct.unpack(">i", data)[0]
