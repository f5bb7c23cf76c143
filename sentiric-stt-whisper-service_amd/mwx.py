"""ctypes binding of the mwx C ABI (include/mwx.h, include/mwx_test.h).

Mirrors the whisper.h subset the reference service binds in
src/stt_engine.cpp (context / state lifecycle, whisper_full_with_state, segment
and token getters) plus the batched entry point mwx_full_batch. Used by the
tests and by bench.py; the service itself binds the same ABI from C++
(see INTEGRATION.md).

The library is loaded from this directory (built in-tree by
__graft_entry__.build()); a missing library raises immediately — there is no
CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# MWX_LIB: an alternative build of the library (same ABI; A/B measurements)
LIB_PATH = os.environ.get("MWX_LIB") or os.path.join(HERE, "libmwx.so")

GGML_F16 = 1
GGML_BF16 = 30
# ggml block-quantized types written by whisper.cpp's quantize tool
GGML_Q4_0 = 2
GGML_Q4_1 = 3
GGML_Q5_0 = 6
GGML_Q5_1 = 7
GGML_Q8_0 = 8
GGML_Q2_K = 10
GGML_Q3_K = 11
GGML_Q4_K = 12
GGML_Q5_K = 13
GGML_Q6_K = 14
GGML_QUANT_TYPES = {"q4_0": GGML_Q4_0, "q4_1": GGML_Q4_1, "q5_0": GGML_Q5_0,
                    "q5_1": GGML_Q5_1, "q8_0": GGML_Q8_0, "q2_k": GGML_Q2_K,
                    "q3_k": GGML_Q3_K, "q4_k": GGML_Q4_K, "q5_k": GGML_Q5_K,
                    "q6_k": GGML_Q6_K}
SAMPLING_GREEDY = 0
SAMPLING_BEAM_SEARCH = 1


class Ahead(C.Structure):
    """mwx_ahead (whisper_ahead): one alignment head."""
    _fields_ = [("n_text_layer", C.c_int), ("n_head", C.c_int)]


class Aheads(C.Structure):
    """mwx_aheads (whisper_aheads)."""
    _fields_ = [("n_heads", C.c_size_t), ("heads", C.POINTER(Ahead))]


class ContextParams(C.Structure):
    _fields_ = [("use_gpu", C.c_bool), ("flash_attn", C.c_bool), ("gpu_device", C.c_int),
                ("compute", C.c_int), ("dtw_token_timestamps", C.c_bool),
                ("dtw_aheads_preset", C.c_int), ("dtw_n_top", C.c_int), ("dtw_aheads", Aheads),
                ("dtw_mem_size", C.c_size_t)]


# enum mwx_alignment_heads_preset (whisper_alignment_heads_preset)
AHEADS_NONE, AHEADS_N_TOP_MOST, AHEADS_CUSTOM = 0, 1, 2
(AHEADS_TINY_EN, AHEADS_TINY, AHEADS_BASE_EN, AHEADS_BASE, AHEADS_SMALL_EN, AHEADS_SMALL,
 AHEADS_MEDIUM_EN, AHEADS_MEDIUM, AHEADS_LARGE_V1, AHEADS_LARGE_V2, AHEADS_LARGE_V3,
 AHEADS_LARGE_V3_TURBO) = range(3, 15)


COMPUTE_MODEL = 0
COMPUTE_MXFP8 = 1  # encoder / cross-K/V GEMMs on MX-fp8 MFMA


class TokenData(C.Structure):
    _fields_ = [
        ("id", C.c_int32), ("tid", C.c_int32), ("p", C.c_float), ("plog", C.c_float),
        ("pt", C.c_float), ("ptsum", C.c_float), ("t0", C.c_int64), ("t1", C.c_int64),
        ("t_dtw", C.c_int64), ("vlen", C.c_float),
    ]


class _Greedy(C.Structure):
    _fields_ = [("best_of", C.c_int)]


class _Beam(C.Structure):
    _fields_ = [("beam_size", C.c_int), ("patience", C.c_float)]


ABORT_CB = C.CFUNCTYPE(C.c_bool, C.c_void_p)

BIAS_MAX_TOKENS = 16
BIAS_MAX_PHRASES = 1024


class BiasPhrase(C.Structure):
    """mwx_bias_phrase: one boosted phrase (contextual biasing)."""
    _fields_ = [("tokens", C.POINTER(C.c_int32)), ("n_tokens", C.c_int), ("boost", C.c_float)]


def bias_phrases(phrases):
    """(array of BiasPhrase or None, objects to keep alive) for an iterable of
    (token ids, boost). Nothing is checked here: the library refuses bad input."""
    items = [(np.ascontiguousarray(t, dtype=np.int32).reshape(-1), float(b)) for t, b in phrases]
    if not items:
        return None, []
    arr = (BiasPhrase * len(items))()
    for i, (t, b) in enumerate(items):
        arr[i].tokens = t.ctypes.data_as(C.POINTER(C.c_int32))
        arr[i].n_tokens = len(t)
        arr[i].boost = b
    return arr, [arr] + [t for t, _ in items]


def with_bias(params: "FullParams", phrases) -> "FullParams":
    """A copy of params with bias_phrases / n_bias_phrases set to the given
    (token ids, boost) pairs. The copy keeps the arrays alive (and the
    caller's params its strings: keep that one too)."""
    p = FullParams.from_buffer_copy(params)
    arr, keep = bias_phrases(phrases)
    p.bias_phrases = arr
    p.n_bias_phrases = 0 if arr is None else len(arr)
    p._bias_keep = (keep, params)
    return p


class FullParams(C.Structure):
    _fields_ = [
        ("strategy", C.c_int), ("n_threads", C.c_int), ("n_max_text_ctx", C.c_int),
        ("offset_ms", C.c_int), ("duration_ms", C.c_int),
        ("translate", C.c_bool), ("no_context", C.c_bool), ("no_timestamps", C.c_bool),
        ("single_segment", C.c_bool), ("print_special", C.c_bool), ("print_progress", C.c_bool),
        ("print_realtime", C.c_bool), ("print_timestamps", C.c_bool),
        ("token_timestamps", C.c_bool), ("thold_pt", C.c_float), ("thold_ptsum", C.c_float),
        ("max_len", C.c_int), ("split_on_word", C.c_bool), ("max_tokens", C.c_int),
        ("audio_ctx", C.c_int), ("tdrz_enable", C.c_bool),
        ("initial_prompt", C.c_char_p), ("prompt_tokens", C.POINTER(C.c_int32)),
        ("prompt_n_tokens", C.c_int),
        ("language", C.c_char_p), ("detect_language", C.c_bool),
        ("suppress_blank", C.c_bool), ("suppress_nst", C.c_bool),
        ("temperature", C.c_float), ("max_initial_ts", C.c_float), ("length_penalty", C.c_float),
        ("temperature_inc", C.c_float), ("entropy_thold", C.c_float),
        ("logprob_thold", C.c_float), ("no_speech_thold", C.c_float),
        ("greedy", _Greedy), ("beam_search", _Beam),
        ("abort_callback", ABORT_CB), ("abort_callback_user_data", C.c_void_p),
        ("bench_fixed_steps", C.c_int),
        ("audio_ctx_fit", C.c_bool),
        ("lang_ids", C.POINTER(C.c_int)),
        ("chunk_language", C.c_int),
        ("bias_phrases", C.POINTER(BiasPhrase)), ("n_bias_phrases", C.c_int),
        ("constraint", C.c_void_p), ("constraint_penalty", C.c_float),
    ]


CHUNK_LANG_PER_CHUNK, CHUNK_LANG_RECORDING = 0, 1


class VadContextParams(C.Structure):
    """mwx_vad_context_params (whisper_vad_context_params)."""
    _fields_ = [("n_threads", C.c_int), ("use_gpu", C.c_bool), ("gpu_device", C.c_int)]


class VadParams(C.Structure):
    """mwx_vad_params (whisper_vad_params): the segment rule's parameters."""
    _fields_ = [("threshold", C.c_float), ("min_speech_duration_ms", C.c_int),
                ("min_silence_duration_ms", C.c_int), ("max_speech_duration_s", C.c_float),
                ("speech_pad_ms", C.c_int), ("samples_overlap", C.c_float)]


class ProsodyParams(C.Structure):
    """mwx_prosody_params = the reference's ProsodyOptions
    (src/prosody_extractor.h:21-27)."""
    _fields_ = [("lpf_alpha", C.c_float), ("gender_threshold", C.c_float),
                ("min_pitch", C.c_float), ("max_pitch", C.c_float)]


# GEMM epilogues (csrc/kernels.h enum Epi) that mwx_test_gemm_enc serves
EPI_ENC_QKV, EPI_GELU, EPI_RES, EPI_CONV2, EPI_CROSS_KV = 0, 1, 2, 3, 5


class TestGemmEncArgs(C.Structure):
    """mwx_test_gemm_enc_args (include/mwx_test.h)."""
    __test__ = False
    _fields_ = ([(n, C.c_int) for n in ("bf16", "epi", "out16", "use_table", "mx", "kv8", "M", "N",
                                        "K", "batch")] +
                [(n, C.c_long) for n in ("lda", "a_bstride", "a_len", "ldc", "c_bstride", "c_off",
                                         "c_len")] +
                [(n, C.c_int) for n in ("L", "H", "d", "ldv", "lcap", "ncap")] +
                [("kscale", C.c_float)] +
                [(n, C.POINTER(C.c_float)) for n in ("a", "w", "bias", "pe")] +
                [("slot", C.POINTER(C.c_int)), ("c16", C.POINTER(C.c_uint16)),
                 ("c32", C.POINTER(C.c_float))] +
                [(n, C.POINTER(C.c_uint16)) for n in ("q", "k", "v")] +
                [(n, C.POINTER(C.c_uint8)) for n in ("k8", "v8", "ks8", "vs8")])


class TestGemmDecArgs(C.Structure):
    """mwx_test_gemm_dec_args (include/mwx_test.h)."""
    __test__ = False
    _fields_ = ([(n, C.c_int) for n in ("bf16", "mode", "w8", "ln", "M", "N", "K", "KS")] +
                [(n, C.POINTER(C.c_float)) for n in ("a", "w")] +
                [(n, C.POINTER(C.c_uint8)) for n in ("wq", "ws")] +
                [(n, C.POINTER(C.c_float)) for n in ("bias", "res", "x_in", "P", "pbias", "ln_w",
                                                     "ln_b")] +
                [("active", C.POINTER(C.c_int)), ("x_out", C.POINTER(C.c_float)),
                 ("ks_out", C.POINTER(C.c_int)), ("out", C.POINTER(C.c_float)),
                 ("out16", C.POINTER(C.c_uint16))])


class TestLogitsConst(C.Structure):
    """mwx_test_logits_const (include/mwx_test.h): the kernels' LogitsConst."""
    __test__ = False
    _fields_ = [(n, C.c_int) for n in ("n_vocab", "eot", "beg", "space_id", "suppress_blank",
                                       "max_initial_tid", "nosp_id")]


# mwx_test_logits_ctl / mwx_test_logits_out as numpy record types
LOGITS_CTL = np.dtype([(n, "<i4") for n in ("active", "sample", "is_initial", "last_ts",
                                            "penult_ts", "has_ts", "seek_delta", "want_probs",
                                            "want_nosp")] + [("temperature", "<f4")])
LOGITS_OUT = np.dtype([("id", "<i4"), ("tid", "<i4")] +
                      [(n, "<f4") for n in ("p", "plog", "pt", "ptsum", "nosp")])


class Prosody(C.Structure):
    """mwx_prosody = AffectiveTags (src/prosody_extractor.h:6-18)."""
    _fields_ = [(n, C.c_float) for n in ("pitch_mean", "pitch_std", "energy_mean", "energy_std",
                                         "spectral_centroid", "zero_crossing_rate", "arousal",
                                         "valence")] + [
        ("speaker_vec", C.c_float * 8), ("gender", C.c_int), ("emotion", C.c_int),
        ("serial_runs", C.c_int), ("reserved", C.c_int)]

    @property
    def gender_proxy(self) -> str:
        return ("?", "M", "F")[self.gender]

    @property
    def emotion_proxy(self) -> str:
        return ("neutral", "excited", "angry", "sad")[self.emotion]


_lib = None

CONSTRAINT_MAX_STATES = 4096
CONSTRAINT_FOLD_CASE = 1
CONSTRAINT_LEADING_SPACE = 2
CONSTRAINT_TRAILING_PUNCT = 4


class Constraint:
    """mwx_constraint (constrained decoding): a byte-level DFA.
    from_dfa / from_choices raise ValueError where the library returns NULL."""

    def __init__(self, ptr):
        self.ptr = ptr

    @staticmethod
    def _decl():
        L = lib()
        u16, u8 = C.POINTER(C.c_uint16), C.POINTER(C.c_uint8)
        L.mwx_constraint_from_dfa.restype = C.c_void_p
        L.mwx_constraint_from_dfa.argtypes = [C.c_int, C.c_int, u16, u8]
        L.mwx_constraint_from_choices.restype = C.c_void_p
        L.mwx_constraint_from_choices.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.c_int]
        L.mwx_constraint_free.restype = None
        L.mwx_constraint_free.argtypes = [C.c_void_p]
        for name in ("n_states", "start"):
            f = getattr(L, "mwx_constraint_" + name)
            f.restype = C.c_int
            f.argtypes = [C.c_void_p]
        L.mwx_constraint_accepting.restype = C.c_int
        L.mwx_constraint_accepting.argtypes = [C.c_void_p, C.c_int]
        L.mwx_constraint_walk.restype = C.c_int
        L.mwx_constraint_walk.argtypes = [C.c_void_p, C.c_int, u8, C.c_int]
        return L

    @classmethod
    def from_dfa(cls, trans, accepting, start: int, n_states=None) -> "Constraint":
        """trans [S][256] state ids, accepting [S] flags."""
        trans = np.ascontiguousarray(trans, dtype=np.uint16)
        accepting = np.ascontiguousarray(accepting, dtype=np.uint8)
        S = int(trans.shape[0]) if n_states is None else int(n_states)
        L = cls._decl()
        ptr = L.mwx_constraint_from_dfa(S, int(start),
                                        trans.ctypes.data_as(C.POINTER(C.c_uint16)),
                                        accepting.ctypes.data_as(C.POINTER(C.c_uint8)))
        if not ptr:
            raise ValueError("mwx_constraint_from_dfa refused the automaton")
        return cls(ptr)

    @classmethod
    def from_choices(cls, texts, flags: int = 0) -> "Constraint":
        """texts: str (UTF-8 encoded) or bytes."""
        bs = [t if isinstance(t, bytes) else t.encode("utf-8") for t in texts]
        arr = (C.c_char_p * max(1, len(bs)))(*bs)
        L = cls._decl()
        ptr = L.mwx_constraint_from_choices(arr, len(bs), int(flags))
        if not ptr:
            raise ValueError("mwx_constraint_from_choices refused the texts")
        return cls(ptr)

    def free(self):
        if self.ptr:
            lib().mwx_constraint_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    @property
    def n_states(self) -> int:
        return self._decl().mwx_constraint_n_states(self.ptr)

    @property
    def start(self) -> int:
        return self._decl().mwx_constraint_start(self.ptr)

    def accepting(self, s: int) -> bool:
        return bool(self._decl().mwx_constraint_accepting(self.ptr, int(s)))

    def walk(self, data: bytes, s=None) -> int:
        """The state after `data` from s (None: the start)."""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        L = self._decl()
        return L.mwx_constraint_walk(self.ptr, self.start if s is None else int(s),
                                     buf.ctypes.data_as(C.POINTER(C.c_uint8)), len(buf))


def with_constraint(params: "FullParams", constraint, penalty=None) -> "FullParams":
    """A copy of params with constraint (a Constraint or None) and, if given,
    constraint_penalty set. The copy keeps the constraint alive (and the
    caller's params its strings: keep that one too)."""
    p = FullParams.from_buffer_copy(params)
    p.constraint = None if constraint is None else constraint.ptr
    if penalty is not None:
        p.constraint_penalty = penalty
    p._con_keep = (constraint, params, getattr(params, "_bias_keep", None))
    return p


def constraint_walk_hook(data: bytes, texts=None, flags: int = 0, trans=None, accepting=None,
                         start: int = 0, from_state: int = -1):
    """mwx_test_constraint_walk (host only): builds the constraint from choices
    (texts) or from a DFA and walks data. Returns (state or -1, accepting flag,
    n_states, n_classes, table bytes)."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    u16, u8 = C.POINTER(C.c_uint16), C.POINTER(C.c_uint8)
    fn = lib().mwx_test_constraint_walk
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.c_int, u16, u8, C.c_int, u8,
                   C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                   C.POINTER(C.c_longlong)]
    acc, ns, nc, nb = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_longlong(-1)
    if texts is not None:
        bs = [t if isinstance(t, bytes) else t.encode("utf-8") for t in texts]
        arr = (C.c_char_p * max(1, len(bs)))(*bs)
        rc = fn(arr, len(bs), int(flags), 0, 0, u16(), u8(), from_state,
                buf.ctypes.data_as(u8), len(buf), C.byref(acc), C.byref(ns), C.byref(nc),
                C.byref(nb))
    else:
        trans = np.ascontiguousarray(trans, dtype=np.uint16)
        accepting = np.ascontiguousarray(accepting, dtype=np.uint8)
        rc = fn(C.POINTER(C.c_char_p)(), 0, 0, int(trans.shape[0]), int(start),
                trans.ctypes.data_as(u16), accepting.ctypes.data_as(u8), from_state,
                buf.ctypes.data_as(u8), len(buf), C.byref(acc), C.byref(ns), C.byref(nc),
                C.byref(nb))
    return rc, acc.value, ns.value, nc.value, nb.value


def bias_state(phrases, hist) -> int:
    """mwx_test_bias_state (host only): the matcher state id after hist."""
    arr, keep = bias_phrases(phrases)
    h = np.ascontiguousarray(hist, dtype=np.int32).reshape(-1)
    fn = lib().mwx_test_bias_state
    ip = C.POINTER(C.c_int32)
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(BiasPhrase), C.c_int, ip, C.c_int]
    rc = fn(arr, 0 if arr is None else len(arr), h.ctypes.data_as(ip), len(h))
    del keep
    return rc


def bias_match(phrases, hist, cap: int = 4096):
    """mwx_test_bias_match (host only): the matcher tables of the (token ids,
    boost) pairs, the state after hist from the root. Returns (rc, {token:
    bias}, table bytes); rc < 0: the refusal code."""
    arr, keep = bias_phrases(phrases)
    h = np.ascontiguousarray(hist, dtype=np.int32).reshape(-1)
    toks = np.zeros(max(cap, 1), np.int32)
    boosts = np.zeros(max(cap, 1), np.float32)
    nbytes = C.c_longlong(-1)
    fn = lib().mwx_test_bias_match
    ip = C.POINTER(C.c_int32)
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(BiasPhrase), C.c_int, ip, C.c_int, ip, C.POINTER(C.c_float), C.c_int,
                   C.POINTER(C.c_longlong)]
    rc = fn(arr, 0 if arr is None else len(arr), h.ctypes.data_as(ip), len(h),
            toks.ctypes.data_as(ip), boosts.ctypes.data_as(C.POINTER(C.c_float)), cap,
            C.byref(nbytes))
    del keep
    n = max(0, min(rc, cap))
    return rc, {int(t): np.float32(b) for t, b in zip(toks[:n], boosts[:n])}, nbytes.value


def lib() -> C.CDLL:
    """Loads libmwx.so (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"mwx: {LIB_PATH} not built (run __graft_entry__.build())")
    L = C.CDLL(LIB_PATH)
    P = C.c_void_p
    L.mwx_context_default_params.restype = ContextParams
    L.mwx_init_from_file_with_params.restype = P
    L.mwx_init_from_file_with_params.argtypes = [C.c_char_p, ContextParams]
    L.mwx_init_state.restype = P
    L.mwx_init_state.argtypes = [P]
    L.mwx_free_state.argtypes = [P]
    L.mwx_free.argtypes = [P]
    L.mwx_full_default_params.restype = FullParams
    L.mwx_full_default_params.argtypes = [C.c_int]
    L.mwx_full_with_state.restype = C.c_int
    L.mwx_full_with_state.argtypes = [P, P, FullParams, C.POINTER(C.c_float), C.c_int]
    fpp = C.POINTER(C.c_float)
    L.mwx_device_buffer.restype = fpp
    L.mwx_device_buffer.argtypes = [P, C.c_size_t]
    L.mwx_device_upload.restype = C.c_int
    L.mwx_device_upload.argtypes = [P, fpp, fpp, C.c_size_t]
    L.mwx_device_buffer_free.restype = None
    L.mwx_device_buffer_free.argtypes = [P, fpp]
    L.mwx_full_batch_pcm16.restype = C.c_int
    L.mwx_full_batch_pcm16.argtypes = [P, C.POINTER(P), FullParams, C.POINTER(C.c_void_p),
                                       C.POINTER(C.c_int), C.c_int]
    L.mwx_full_batch.restype = C.c_int
    L.mwx_full_batch.argtypes = [P, C.POINTER(P), FullParams, C.POINTER(C.POINTER(C.c_float)),
                                 C.POINTER(C.c_int), C.c_int]
    L.mwx_full_n_segments_from_state.restype = C.c_int
    L.mwx_full_n_segments_from_state.argtypes = [P]
    L.mwx_full_get_segment_text_from_state.restype = C.c_char_p
    L.mwx_full_get_segment_text_from_state.argtypes = [P, C.c_int]
    for n in ("t0", "t1"):
        f = getattr(L, f"mwx_full_get_segment_{n}_from_state")
        f.restype = C.c_int64
        f.argtypes = [P, C.c_int]
    L.mwx_full_get_segment_speaker_turn_next_from_state.restype = C.c_bool
    L.mwx_full_get_segment_speaker_turn_next_from_state.argtypes = [P, C.c_int]
    L.mwx_full_get_segment_no_speech_prob_from_state.restype = C.c_float
    L.mwx_full_get_segment_no_speech_prob_from_state.argtypes = [P, C.c_int]
    L.mwx_full_n_tokens_from_state.restype = C.c_int
    L.mwx_full_n_tokens_from_state.argtypes = [P, C.c_int]
    L.mwx_full_get_token_data_from_state.restype = TokenData
    L.mwx_full_get_token_data_from_state.argtypes = [P, C.c_int, C.c_int]
    L.mwx_full_lang_id_from_state.restype = C.c_int
    L.mwx_full_lang_id_from_state.argtypes = [P]
    L.mwx_token_to_str.restype = C.c_char_p
    L.mwx_token_to_str.argtypes = [P, C.c_int32]
    for n in ("eot", "sot", "beg", "not", "nosp", "transcribe", "translate"):
        f = getattr(L, f"mwx_token_{n}")
        f.restype = C.c_int32
        f.argtypes = [P]
    for n in ("n_vocab", "n_text_ctx", "n_audio_ctx", "n_mels", "is_multilingual", "model_wtype"):
        f = getattr(L, f"mwx_{n}")
        f.restype = C.c_int
        f.argtypes = [P]
    L.mwx_audio_ctx_for.restype = C.c_int
    L.mwx_audio_ctx_for.argtypes = [P, C.c_int, C.c_int, C.c_int, C.c_bool]
    L.mwx_model_quantize.restype = C.c_int
    L.mwx_model_quantize.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    L.mwx_write_synthetic_model.restype = C.c_int
    L.mwx_write_synthetic_model.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_uint64]
    L.mwx_perf_enable.restype = None
    L.mwx_perf_enable.argtypes = [P, C.c_char_p]
    L.mwx_perf_read.restype = C.c_int
    L.mwx_perf_read.argtypes = [P, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    L.mwx_perf_read_class.restype = C.c_int
    L.mwx_perf_read_class.argtypes = [P, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    L.mwx_tokenize.restype = C.c_int
    L.mwx_tokenize.argtypes = [P, C.c_char_p, C.POINTER(C.c_int32), C.c_int]
    L.mwx_test_mel.restype = C.c_int
    L.mwx_test_mel.argtypes = [P, P, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_float), C.c_long]
    L.mwx_test_encode.restype = C.c_int
    L.mwx_test_encode.argtypes = [P, P, C.POINTER(C.c_float), C.c_int, C.c_int,
                                  C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.mwx_test_encode_ctx.restype = C.c_int
    L.mwx_test_encode_ctx.argtypes = [P, P, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int,
                                      C.POINTER(C.c_float), C.POINTER(C.c_float),
                                      C.POINTER(C.c_float)]
    L.mwx_test_decode.restype = C.c_int
    L.mwx_test_decode.argtypes = [P, P, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_float)]
    L.mwx_test_decode_last.restype = C.c_int
    L.mwx_test_decode_last.argtypes = [P, P, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_float)]
    L.mwx_test_decode_last_prefill.restype = C.c_int
    L.mwx_test_decode_last_prefill.argtypes = [P, P, C.POINTER(C.c_int), C.c_int,
                                               C.POINTER(C.c_float)]
    L.mwx_test_self_kv.restype = C.c_int
    L.mwx_test_self_kv.argtypes = [P, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.mwx_test_dequantize.restype = C.c_int
    L.mwx_test_dequantize.argtypes = [C.c_int, C.c_void_p, C.c_long, C.POINTER(C.c_float)]
    L.mwx_test_decode_counters.restype = C.c_int
    L.mwx_test_decode_counters.argtypes = [P, C.POINTER(C.c_long), C.POINTER(C.c_long), C.c_int]
    L.mwx_test_encode_dump.restype = C.c_int
    L.mwx_test_encode_dump.argtypes = [P, P, C.POINTER(C.c_float), C.c_int, C.c_int,
                                       C.POINTER(C.c_float), C.POINTER(C.c_void_p)]
    L.mwx_test_window_counters.restype = C.c_int
    L.mwx_test_window_counters.argtypes = [P, C.POINTER(C.c_long), C.POINTER(C.c_long),
                                           C.POINTER(C.c_long), C.c_int]
    L.mwx_test_runahead_fallbacks.restype = C.c_long
    L.mwx_test_runahead_fallbacks.argtypes = [P, C.c_int]
    L.mwx_test_set_xattn_mfs.restype = C.c_int
    L.mwx_test_set_xattn_mfs.argtypes = [C.c_int]
    L.mwx_test_set_dec_shared.restype = C.c_int
    L.mwx_test_set_dec_shared.argtypes = [C.c_int]
    L.mwx_test_set_gemm_8ph.restype = C.c_int
    L.mwx_test_set_ln_fold.restype = C.c_int
    L.mwx_test_set_ln_fold.argtypes = [C.c_int]
    L.mwx_test_mx_widen.restype = C.c_int
    L.mwx_test_mx_widen.argtypes = [P, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.mwx_test_set_gemm_8ph.argtypes = [C.c_int]
    L.mwx_test_set_ra_mismatch.restype = C.c_long
    L.mwx_test_set_ra_mismatch.argtypes = [C.c_long]
    u8p = C.POINTER(C.c_uint8)
    L.mwx_test_xattn_mx.restype = C.c_int
    L.mwx_test_xattn_mx.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, fpp, u8p, u8p,
                                    u8p, u8p, fpp]
    L.mwx_test_sample_draws.restype = C.c_int
    L.mwx_test_sample_draws.argtypes = [P, fpp, fpp, C.c_int, C.c_int, C.POINTER(C.c_double),
                                        C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int,
                                        C.POINTER(C.c_int), C.POINTER(C.c_double)]
    ipp, u16p = C.POINTER(C.c_int), C.POINTER(C.c_uint16)
    L.mwx_test_dec_attn.restype = C.c_int
    L.mwx_test_dec_attn.argtypes = [P] + [C.c_int] * 10 + [fpp, fpp, C.c_float, C.c_float,
                                                          C.c_float, u16p, u16p, ipp, ipp, ipp,
                                                          ipp, ipp, C.c_int, fpp]
    L.mwx_test_gemm_dec.restype = C.c_int
    L.mwx_test_gemm_dec.argtypes = [P] + [C.c_int] * 5 + [fpp, fpp, fpp, fpp, ipp, fpp]
    L.mwx_resample_max_frames.restype = C.c_long
    L.mwx_resample_max_frames.argtypes = [C.c_int, C.c_int, C.c_int]
    L.mwx_resample.restype = C.c_int
    L.mwx_resample.argtypes = [P, P, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.mwx_prosody_default_params.restype = ProsodyParams
    L.mwx_prosody_default_params.argtypes = []
    i64p = C.POINTER(C.c_int64)
    L.mwx_prosody_batch.restype = C.c_int
    L.mwx_prosody_batch.argtypes = [P, P, fpp, C.c_int64, i64p, i64p, C.c_int, C.c_int,
                                    C.POINTER(ProsodyParams), C.POINTER(Prosody)]
    L.mwx_prosody_batch_device.restype = C.c_int
    L.mwx_prosody_batch_device.argtypes = [P, P, C.c_void_p, C.c_void_p, C.c_int, C.c_int64,
                                           C.c_int, C.POINTER(ProsodyParams), C.c_void_p]
    L.mwx_vad_default_context_params.restype = VadContextParams
    L.mwx_vad_default_context_params.argtypes = []
    L.mwx_vad_init_from_file_with_params.restype = P
    L.mwx_vad_init_from_file_with_params.argtypes = [C.c_char_p, VadContextParams]
    L.mwx_vad_free.restype = None
    L.mwx_vad_free.argtypes = [P]
    L.mwx_vad_detect_speech.restype = C.c_bool
    L.mwx_vad_detect_speech.argtypes = [P, C.c_void_p, C.c_int]
    L.mwx_vad_n_probs.restype = C.c_int
    L.mwx_vad_n_probs.argtypes = [P]
    L.mwx_vad_probs.restype = fpp
    L.mwx_vad_probs.argtypes = [P]
    L.mwx_vad_n_chunks.restype = C.c_int
    L.mwx_vad_n_chunks.argtypes = [C.c_int]
    L.mwx_vad_detect_speech_batch.restype = C.c_int
    L.mwx_vad_detect_speech_batch.argtypes = [P, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int,
                                              fpp, C.POINTER(C.c_int)]
    L.mwx_vad_last_kernel_ms.restype = C.c_int
    L.mwx_vad_last_kernel_ms.argtypes = [P, fpp, fpp]
    L.mwx_write_synthetic_vad_model.restype = C.c_int
    L.mwx_write_synthetic_vad_model.argtypes = [C.c_char_p, C.c_uint64]
    ip = C.POINTER(C.c_int)
    L.mwx_vad_default_params.restype = VadParams
    L.mwx_vad_default_params.argtypes = []
    L.mwx_vad_segments_from_probs.restype = P
    L.mwx_vad_segments_from_probs.argtypes = [P, VadParams]
    L.mwx_vad_segments_from_samples.restype = P
    L.mwx_vad_segments_from_samples.argtypes = [P, VadParams, C.c_void_p, C.c_int]
    L.mwx_vad_segments_n_segments.restype = C.c_int
    L.mwx_vad_segments_n_segments.argtypes = [P]
    for n in ("t0", "t1"):
        f = getattr(L, f"mwx_vad_segments_get_segment_{n}")
        f.restype = C.c_float
        f.argtypes = [P, C.c_int]
    L.mwx_vad_free_segments.restype = None
    L.mwx_vad_free_segments.argtypes = [P]
    L.mwx_vad_trim_batch.restype = P
    L.mwx_vad_trim_batch.argtypes = [P, VadParams, C.POINTER(C.c_void_p), ip, C.c_int]
    L.mwx_vad_trimmed_n_clips.restype = C.c_int
    L.mwx_vad_trimmed_n_clips.argtypes = [P]
    L.mwx_vad_trimmed_n_segments.restype = C.c_int
    L.mwx_vad_trimmed_n_segments.argtypes = [P, C.c_int]
    L.mwx_vad_trimmed_segment.restype = C.c_int
    L.mwx_vad_trimmed_segment.argtypes = [P, C.c_int, C.c_int, i64p, i64p]
    L.mwx_vad_trimmed_n_samples.restype = C.c_int64
    L.mwx_vad_trimmed_n_samples.argtypes = [P, C.c_int]
    L.mwx_vad_trimmed_pcm.restype = C.c_void_p
    L.mwx_vad_trimmed_pcm.argtypes = [P, C.c_int]
    L.mwx_vad_trimmed_map_time.restype = C.c_int64
    L.mwx_vad_trimmed_map_time.argtypes = [P, C.c_int, C.c_int64, C.c_bool]
    L.mwx_vad_trimmed_free.restype = None
    L.mwx_vad_trimmed_free.argtypes = [P]
    L.mwx_vad_last_trim_kernel_ms.restype = C.c_int
    L.mwx_vad_last_trim_kernel_ms.argtypes = [P, fpp, fpp]
    L.mwx_full_batch_trimmed.restype = C.c_int
    L.mwx_full_batch_trimmed.argtypes = [P, C.POINTER(P), FullParams, C.POINTER(P), ip, C.c_int]
    L.mwx_test_vad_segments.restype = C.c_int
    L.mwx_test_vad_segments.argtypes = [P, C.POINTER(VadParams), fpp, ip, ip, C.c_int, ip, i64p,
                                        i64p, i64p, ip]
    L.mwx_test_vad_trimmed_pcm.restype = C.c_int64
    L.mwx_test_vad_trimmed_pcm.argtypes = [P, C.c_int, fpp, C.c_int64]
    L.mwx_vad_trim_batch_chunked.restype = P
    L.mwx_vad_trim_batch_chunked.argtypes = [P, VadParams, C.c_float, C.POINTER(C.c_void_p), ip,
                                             C.c_int]
    L.mwx_vad_trimmed_n_chunks.restype = C.c_int
    L.mwx_vad_trimmed_n_chunks.argtypes = [P, C.c_int]
    L.mwx_vad_trimmed_chunk.restype = C.c_int
    L.mwx_vad_trimmed_chunk.argtypes = [P, C.c_int, C.c_int, ip, ip, i64p, i64p]
    L.mwx_vad_trimmed_chunk_map_time.restype = C.c_int64
    L.mwx_vad_trimmed_chunk_map_time.argtypes = [P, C.c_int, C.c_int, C.c_int64, C.c_bool]
    L.mwx_vad_last_chunk_kernel_ms.restype = C.c_int
    L.mwx_vad_last_chunk_kernel_ms.argtypes = [P, fpp]
    L.mwx_full_batch_chunked.restype = C.c_int
    L.mwx_full_batch_chunked.argtypes = [P, C.POINTER(P), FullParams, C.POINTER(P), ip, C.c_int,
                                         C.c_int]
    L.mwx_test_vad_chunks.restype = C.c_int
    L.mwx_test_vad_chunks.argtypes = [P, C.POINTER(VadParams), i64p, fpp, ip, ip, C.c_int, ip,
                                      i64p, ip]
    L.mwx_vad_stream_init.restype = P
    L.mwx_vad_stream_init.argtypes = [P, VadParams]
    L.mwx_vad_stream_free.restype = None
    L.mwx_vad_stream_free.argtypes = [P]
    L.mwx_vad_stream_reset.restype = C.c_int
    L.mwx_vad_stream_reset.argtypes = [P]
    L.mwx_vad_stream_feed_batch.restype = C.c_int
    L.mwx_vad_stream_feed_batch.argtypes = [P, C.POINTER(P), C.POINTER(C.c_void_p), ip, C.c_int]
    L.mwx_vad_stream_finish.restype = C.c_int
    L.mwx_vad_stream_finish.argtypes = [P]
    L.mwx_vad_stream_n_samples.restype = C.c_int64
    L.mwx_vad_stream_n_samples.argtypes = [P]
    L.mwx_vad_stream_n_probs.restype = C.c_int
    L.mwx_vad_stream_n_probs.argtypes = [P]
    L.mwx_vad_stream_probs.restype = fpp
    L.mwx_vad_stream_probs.argtypes = [P]
    L.mwx_vad_stream_max_prob.restype = C.c_float
    L.mwx_vad_stream_max_prob.argtypes = [P]
    L.mwx_vad_stream_n_segments.restype = C.c_int
    L.mwx_vad_stream_n_segments.argtypes = [P]
    L.mwx_vad_stream_segment.restype = C.c_int
    L.mwx_vad_stream_segment.argtypes = [P, C.c_int, i64p, i64p, i64p]
    L.mwx_vad_stream_in_speech.restype = C.c_bool
    L.mwx_vad_stream_in_speech.argtypes = [P]
    L.mwx_vad_stream_last_kernel_ms.restype = C.c_int
    L.mwx_vad_stream_last_kernel_ms.argtypes = [P, fpp, fpp, fpp]
    L.mwx_test_vad_stream_scan.restype = C.c_int
    L.mwx_test_vad_stream_scan.argtypes = [P, C.POINTER(VadParams), fpp, C.c_int, ip, C.c_int, ip,
                                           i64p, i64p]
    _lib = L
    return L


def fptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class DevicePCM:
    """f32 PCM in a device buffer of the context's GPU (mwx_device_buffer)."""

    def __init__(self, ctx: "Context", pcm: np.ndarray):
        a = np.ascontiguousarray(pcm, dtype=np.float32)
        self.ctx, self.n = ctx, len(a)
        self.ptr = lib().mwx_device_buffer(ctx.ctx, max(1, self.n))
        if not self.ptr:
            raise MemoryError("mwx_device_buffer failed")
        if lib().mwx_device_upload(ctx.ctx, self.ptr, fptr(a), self.n) != 0:
            raise RuntimeError("mwx_device_upload failed")

    def free(self):
        if self.ptr:
            lib().mwx_device_buffer_free(self.ctx.ctx, self.ptr)
            self.ptr = None


def write_synthetic_model(path: str, arch: str, wtype: int = GGML_F16, seed: int = 0) -> None:
    rc = lib().mwx_write_synthetic_model(path.encode(), arch.encode(), wtype, seed)
    if rc != 0:
        raise RuntimeError(f"mwx_write_synthetic_model failed ({rc})")


def write_synthetic_vad_model(path: str, seed: int = 0) -> None:
    """mwx_write_synthetic_vad_model: a seeded Silero-v5-shaped VAD model."""
    rc = lib().mwx_write_synthetic_vad_model(path.encode(), seed)
    if rc != 0:
        raise RuntimeError(f"mwx_write_synthetic_vad_model failed ({rc})")


def set_xattn_mfs(on: Optional[bool]) -> int:
    """mwx_test_set_xattn_mfs: the MX-fp8 grouped cross-attention on MFMA
    (True) or v_dot2 (False); None: the MWX_XATTN_MFS default."""
    return lib().mwx_test_set_xattn_mfs(-1 if on is None else int(bool(on)))


def set_dec_shared(on: Optional[bool]) -> int:
    """mwx_test_set_dec_shared: decode GEMMs at > 64 rows through the
    shared-A kernels (True) or the per-strip grids (False); None: the
    MWX_DEC_SHARED default."""
    return lib().mwx_test_set_dec_shared(-1 if on is None else int(bool(on)))


def set_gemm_8ph(on: Optional[bool]) -> int:
    """mwx_test_set_gemm_8ph: the encoder GEMM's 8-phase main loop (True) or
    the 2-stage ring (False); None: the MWX_GEMM_8PH default."""
    return lib().mwx_test_set_gemm_8ph(-1 if on is None else int(bool(on)))


def set_ln_fold(on: Optional[bool]) -> int:
    """mwx_test_set_ln_fold: the decode LayerNorms folded into the next
    split-K GEMM at one row (True) or launched separately (False); None: the
    MWX_LN_FOLD default (on)."""
    return lib().mwx_test_set_ln_fold(-1 if on is None else int(bool(on)))


def set_ra_mismatch(step: Optional[int]) -> int:
    """mwx_test_set_ra_mismatch: treat run-ahead step `step` of later attempts
    as a device/host disagreement (None: back to MWX_TEST_RA_MISMATCH, -1: off)."""
    return lib().mwx_test_set_ra_mismatch(-2 if step is None else int(step))


def set_score_rows_cap(rows: int = 0) -> int:
    """mwx_test_set_score_rows_cap: rows per block of align_batch's logits
    buffer (0: the default, 256). Returns the previous value."""
    fn = lib().mwx_test_set_score_rows_cap
    fn.restype = C.c_int
    fn.argtypes = [C.c_int]
    return fn(int(rows))


def lang_max_id() -> int:
    fn = lib().mwx_lang_max_id
    fn.restype = C.c_int
    fn.argtypes = []
    return fn()


def lang_id(code: str) -> int:
    fn = lib().mwx_lang_id
    fn.restype = C.c_int
    fn.argtypes = [C.c_char_p]
    return fn(code.encode())


def lang_str(i: int) -> str:
    fn = lib().mwx_lang_str
    fn.restype = C.c_char_p
    fn.argtypes = [C.c_int]
    s = fn(int(i))
    return s.decode() if s else ""


def stt_lib() -> C.CDLL:
    """libmwx_stt.so (the host SttEngine's C glue) with the alignment calls typed."""
    L = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "libmwx_stt.so"))
    L.mwx_stt_new.restype = C.c_void_p
    L.mwx_stt_new.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_char_p,
                              C.c_int, C.c_int]
    L.mwx_stt_free.argtypes = [C.c_void_p]
    L.mwx_stt_align_pcm16.restype = C.c_int
    L.mwx_stt_align_pcm16.argtypes = [C.c_void_p, C.POINTER(C.c_int16), C.c_int, C.c_int,
                                      C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_int]
    L.mwx_stt_detect_language_pcm16.restype = C.c_int
    L.mwx_stt_detect_language_pcm16.argtypes = [C.c_void_p, C.POINTER(C.c_int16), C.c_int, C.c_int,
                                                C.c_int, C.c_char_p, C.c_int]
    L.mwx_stt_set_chunk_language_recording.restype = C.c_int
    L.mwx_stt_set_chunk_language_recording.argtypes = [C.c_void_p, C.c_int]
    return L


def stt_detect_language_pcm16(L: C.CDLL, eng, pcm16: np.ndarray, sample_rate: int,
                              top_k: int = 0) -> List[tuple]:
    """SttEngine::detect_language_pcm16 through mwx_stt_detect_language_pcm16:
    [(language code, probability as np.float32)], best first (floats exact:
    they cross as f32 bit patterns)."""
    import json
    pcm16 = np.ascontiguousarray(pcm16, dtype=np.int16)
    cap = 1 << 16
    buf = C.create_string_buffer(cap)
    rc = L.mwx_stt_detect_language_pcm16(eng, pcm16.ctypes.data_as(C.POINTER(C.c_int16)),
                                         len(pcm16), sample_rate, int(top_k), buf, cap)
    if rc < 0:
        raise RuntimeError(f"mwx_stt_detect_language_pcm16 failed ({rc})")
    return [(bytes.fromhex(r["language"]).decode(), np.array([r["p"]], np.uint32).view(np.float32)[0])
            for r in json.loads(buf.value.decode())]


def _align_json(r: dict) -> dict:
    f32 = lambda u: float(np.array([u], np.uint32).view(np.float32)[0])
    unhex = lambda s: bytes.fromhex(s).decode("utf-8", "replace")
    out = dict(ok=bool(r["ok"]), text=unhex(r["text"]), language=unhex(r["language"]),
               avg_logprob=f32(r["avg_logprob"]), eot_logprob=f32(r["eot_logprob"]),
               n_agree=r["n_agree"], tokens=[])
    for t in r["tokens"]:
        out["tokens"].append(dict(id=t["id"], p=f32(t["p"]), plog=f32(t["plog"]), t=t["t"],
                                  top_id=t["top_id"], top_plog=f32(t["top_plog"]),
                                  text=unhex(t["text"]), top_text=unhex(t["top_text"])))
    return out


def stt_align_pcm16(L: C.CDLL, eng, pcm16: np.ndarray, sample_rate: int, text: str,
                    language: str = "", translate: bool = False) -> dict:
    """SttEngine::align_pcm16 through mwx_stt_align_pcm16: the AlignmentResult
    as a dict (floats exact: they cross as f32 bit patterns)."""
    import json
    pcm16 = np.ascontiguousarray(pcm16, dtype=np.int16)
    cap = 1 << 20
    buf = C.create_string_buffer(cap)
    rc = L.mwx_stt_align_pcm16(eng, pcm16.ctypes.data_as(C.POINTER(C.c_int16)), len(pcm16),
                               sample_rate, text.encode(), language.encode(), int(translate), buf,
                               cap)
    if rc < 0:
        raise RuntimeError(f"mwx_stt_align_pcm16 failed ({rc})")
    return _align_json(json.loads(buf.value.decode()))


def dequantize(qtype: int, raw: bytes, n: int) -> np.ndarray:
    """mwx_test_dequantize: the engine's load-time dequantizer (host only)."""
    out = np.empty(n, np.float32)
    buf = np.frombuffer(raw, np.uint8)
    rc = lib().mwx_test_dequantize(qtype, buf.ctypes.data, n, out.ctypes.data_as(C.POINTER(C.c_float)))
    if rc != 0:
        raise ValueError(f"mwx_test_dequantize({qtype}, n={n}) returned {rc}")
    return out


def mx_quantize_rows(x: np.ndarray):
    """mwx_test_mx_quantize_rows: the load-time MX-fp8 quantizer (host only).
    x [rows][K] f32 -> (e4m3fn codes uint8 [rows][K], E8M0 scales [rows][K/32])."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    rows, K = x.shape
    q = np.empty((rows, K), np.uint8)
    s = np.empty((rows, K // 32), np.uint8)
    fn = lib().mwx_test_mx_quantize_rows
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_float), C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    rc = fn(x.ctypes.data_as(C.POINTER(C.c_float)), rows, K, q.ctypes.data, s.ctypes.data)
    if rc != 0:
        raise ValueError(f"mwx_test_mx_quantize_rows(rows={rows}, K={K}) returned {rc}")
    return q, s


def quantize_model(in_path: str, out_path: str, qtype: int) -> None:
    """mwx_model_quantize: whisper.cpp `quantize` tool rules."""
    rc = lib().mwx_model_quantize(in_path.encode(), out_path.encode(), qtype)
    if rc != 0:
        raise RuntimeError(f"mwx_model_quantize failed ({rc})")


def synth_pcm16(k: int, n: int = 480000, sr: int = 16000) -> np.ndarray:
    """Deterministic synthetic speech-like clip: 3 harmonic
    voices (F0 90-260 Hz, 8 harmonics with 1/h amplitude), 2-6 Hz amplitude
    modulation, white noise at -30 dBFS, peak 0.5, int16."""
    rng = np.random.default_rng(0x5EED0000 + k)
    t = np.arange(n, dtype=np.float64) / sr
    sig = np.zeros(n)
    for _ in range(3):
        f0 = rng.uniform(90.0, 260.0)
        rate = rng.uniform(2.0, 6.0)
        ph = rng.uniform(0, 2 * np.pi, size=9)
        voice = sum(np.sin(2 * np.pi * h * f0 * t + ph[h]) / h for h in range(1, 9))
        env = 0.5 * (1.0 + np.sin(2 * np.pi * rate * t + ph[0]))
        sig += env * voice
    sig /= np.max(np.abs(sig))
    sig += rng.normal(0.0, 10 ** (-30 / 20), size=n)
    sig *= 0.5 / np.max(np.abs(sig))
    return np.round(sig * 32767).astype(np.int16)


def pcm16_to_f32(pcm16: np.ndarray) -> np.ndarray:
    """SttEngine::transcribe_pcm16 conversion (src/stt_engine.cpp:123)."""
    return (pcm16.astype(np.float32) / np.float32(32768.0)).astype(np.float32)


@dataclass
class Token:
    id: int
    tid: int
    p: float
    plog: float
    pt: float
    ptsum: float
    t0: int
    t1: int
    text: str
    t_dtw: int = -1


@dataclass
class Segment:
    t0: int
    t1: int
    text: str
    no_speech_prob: float
    speaker_turn_next: bool
    tokens: List[Token] = field(default_factory=list)


class Context:
    """mwx_context + a pool of mwx_state objects."""

    def __init__(self, model_path: str, device: int = 0, compute: int = COMPUTE_MODEL,
                 dtw_preset: int = AHEADS_NONE, dtw_heads=None, dtw_n_top: int = -1):
        """dtw_preset != AHEADS_NONE turns DTW token timestamps on
        (mwx_context_params.dtw_token_timestamps): AHEADS_CUSTOM with dtw_heads
        = [(layer, head), ...], AHEADS_N_TOP_MOST with dtw_n_top, or a model
        preset."""
        L = lib()
        cp = L.mwx_context_default_params()
        cp.gpu_device = device
        cp.compute = compute
        if dtw_preset != AHEADS_NONE:
            cp.dtw_token_timestamps = True
            cp.dtw_aheads_preset = dtw_preset
            cp.dtw_n_top = dtw_n_top
            if dtw_heads is not None:
                arr = (Ahead * max(1, len(dtw_heads)))(*[Ahead(l, h) for l, h in dtw_heads])
                cp.dtw_aheads.n_heads = len(dtw_heads)
                cp.dtw_aheads.heads = arr
        self.ctx = L.mwx_init_from_file_with_params(model_path.encode(), cp)
        if not self.ctx:
            raise RuntimeError(f"mwx_init_from_file_with_params failed for {model_path}")
        self.states: List[int] = []

    def close(self):
        L = lib()
        for s in self.states:
            L.mwx_free_state(s)
        self.states = []
        if self.ctx:
            L.mwx_free(self.ctx)
            self.ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def state(self, i: int = 0) -> int:
        while len(self.states) <= i:
            s = lib().mwx_init_state(self.ctx)
            if not s:
                raise RuntimeError("mwx_init_state failed")
            self.states.append(s)
        return self.states[i]

    @staticmethod
    def default_params(strategy: int = SAMPLING_GREEDY) -> FullParams:
        return lib().mwx_full_default_params(strategy)

    def _lang_params(self, params: FullParams, lang_ids, n: int) -> FullParams:
        """params, or a copy of it with FullParams.lang_ids set to the n given
        per-entry language ids (< 0: the entry follows params.language)."""
        if lang_ids is None:
            return params
        ids = [int(i) for i in lang_ids]
        assert len(ids) == n, (len(ids), n)
        arr = (C.c_int * n)(*ids)
        p = FullParams.from_buffer_copy(params)  # (the caller's params keeps its strings alive)
        p.lang_ids = arr
        self._keep_ids = arr
        return p

    def full(self, pcm: np.ndarray, params: FullParams, state_index: int = 0,
             lang_id: Optional[int] = None) -> int:
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        params = self._lang_params(params, None if lang_id is None else [lang_id], 1)
        return lib().mwx_full_with_state(self.ctx, self.state(state_index), params, fptr(pcm),
                                         len(pcm))

    def full_batch(self, pcms: Sequence[np.ndarray], params: FullParams, lang_ids=None) -> int:
        return self.full_batch_states(pcms, params, range(len(pcms)), lang_ids=lang_ids)

    def full_batch_pcm16(self, pcms: Sequence[np.ndarray], params: FullParams,
                         lang_ids=None) -> int:
        """mwx_full_batch_pcm16: int16 PCM converted on the device."""
        n = len(pcms)
        params = self._lang_params(params, lang_ids, n)
        arrs = [np.ascontiguousarray(p, dtype=np.int16) for p in pcms]
        states = (C.c_void_p * n)(*[self.state(i) for i in range(n)])
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
        lens = (C.c_int * n)(*[len(a) for a in arrs])
        self._keep = arrs
        return lib().mwx_full_batch_pcm16(self.ctx, states, params, ptrs, lens, n)

    def full_batch_states(self, pcms: Sequence[np.ndarray], params: FullParams,
                          state_indices: Sequence[int], lang_ids=None) -> int:
        n = len(pcms)
        params = self._lang_params(params, lang_ids, n)
        arrs = [np.ascontiguousarray(p, dtype=np.float32) for p in pcms]
        states = (C.c_void_p * n)(*[self.state(i) for i in state_indices])
        ptrs = (C.POINTER(C.c_float) * n)(*[fptr(a) for a in arrs])
        lens = (C.c_int * n)(*[len(a) for a in arrs])
        self._keep = arrs
        return lib().mwx_full_batch(self.ctx, states, params, ptrs, lens, n)

    def upload(self, pcm: np.ndarray) -> "DevicePCM":
        """Copies PCM into a buffer on this context's GPU (HBM-resident input)."""
        return DevicePCM(self, pcm)

    def full_batch_device(self, bufs: Sequence["DevicePCM"], params: FullParams,
                          state0: int = 0) -> int:
        """Batch over PCM already resident in this GPU's memory: no PCIe transfer.
        Clip i runs on state state0 + i (state0 owns the batch's workspace and
        stream, so batches on disjoint state ranges may run concurrently)."""
        n = len(bufs)
        states = (C.c_void_p * n)(*[self.state(state0 + i) for i in range(n)])
        ptrs = (C.POINTER(C.c_float) * n)(*[b.ptr for b in bufs])
        ln = (C.c_int * n)(*[b.n for b in bufs])
        return lib().mwx_full_batch(self.ctx, states, params, ptrs, ln, n)

    def full_batch_trimmed(self, trimmed: Sequence["VadTrimmed"], clip_index: Sequence[int],
                           params: FullParams, state0: int = 0, lang_ids=None) -> int:
        """mwx_full_batch_trimmed: entry b = clip clip_index[b] of trimmed[b], on
        state state0 + b; the getters then return times of the original clips."""
        n = len(trimmed)
        params = self._lang_params(params, lang_ids, n)
        states = (C.c_void_p * n)(*[self.state(state0 + i) for i in range(n)])
        objs = (C.c_void_p * n)(*[t.t for t in trimmed])
        idx = (C.c_int * n)(*clip_index)
        return lib().mwx_full_batch_trimmed(self.ctx, states, params, objs, idx, n)

    def full_batch_chunked(self, trimmed: Sequence["VadTrimmed"], clip_index: Sequence[int],
                           params: FullParams, max_batch: int = 32, state0: int = 0,
                           lang_ids=None) -> int:
        """mwx_full_batch_chunked: as full_batch_trimmed, every chunk of every
        entry decoded as a batch entry of its own, at most max_batch per run."""
        n = len(trimmed)
        params = self._lang_params(params, lang_ids, n)
        states = (C.c_void_p * n)(*[self.state(state0 + i) for i in range(n)])
        objs = (C.c_void_p * n)(*[t.t for t in trimmed])
        idx = (C.c_int * n)(*clip_index)
        return lib().mwx_full_batch_chunked(self.ctx, states, params, objs, idx, n, max_batch)

    def segments(self, state_index: int = 0) -> List[Segment]:
        L = lib()
        s = self.state(state_index)
        out = []
        for i in range(L.mwx_full_n_segments_from_state(s)):
            seg = Segment(
                t0=L.mwx_full_get_segment_t0_from_state(s, i),
                t1=L.mwx_full_get_segment_t1_from_state(s, i),
                text=L.mwx_full_get_segment_text_from_state(s, i).decode("utf-8", "replace"),
                no_speech_prob=L.mwx_full_get_segment_no_speech_prob_from_state(s, i),
                speaker_turn_next=L.mwx_full_get_segment_speaker_turn_next_from_state(s, i),
            )
            for j in range(L.mwx_full_n_tokens_from_state(s, i)):
                td = L.mwx_full_get_token_data_from_state(s, i, j)
                seg.tokens.append(Token(td.id, td.tid, td.p, td.plog, td.pt, td.ptsum, td.t0,
                                        td.t1, L.mwx_token_to_str(self.ctx, td.id).decode(
                                            "utf-8", "replace"), td.t_dtw))
            out.append(seg)
        return out

    def token_records(self, state_index: int = 0) -> List[tuple]:
        """(id, t0, t1, p) of every token of every segment, in order: the
        per-token whisper.h accessors only (no text), for the gather."""
        L = lib()
        s = self.state(state_index)
        out = []
        for i in range(L.mwx_full_n_segments_from_state(s)):
            for j in range(L.mwx_full_n_tokens_from_state(s, i)):
                td = L.mwx_full_get_token_data_from_state(s, i, j)
                out.append((td.id, td.t0, td.t1, td.p))
        return out

    def lang_id(self, state_index: int = 0) -> int:
        return lib().mwx_full_lang_id_from_state(self.state(state_index))

    def lang_probs(self, state_index: int = 0) -> np.ndarray:
        """mwx_full_lang_probs_from_state: probs[id] of the detection pass of the
        state's last call, f32 [mwx_lang_max_id() + 1]; empty when that call
        did not detect."""
        fn = lib().mwx_full_lang_probs_from_state
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int]
        out = np.zeros(lang_max_id() + 1, np.float32)
        n = fn(self.state(state_index), fptr(out), out.size)
        if n < 0:
            raise RuntimeError(f"mwx_full_lang_probs_from_state returned {n}")
        return out[:n]

    def lang_keep(self, on: bool = True, state_index: int = 0) -> None:
        """mwx_test_lang_keep: the state keeps the language-logit row of its
        detection passes for lang_last()."""
        fn = lib().mwx_test_lang_keep
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int]
        fn(self.state(state_index), 1 if on else 0)

    def lang_last(self, state_index: int = 0) -> np.ndarray:
        """mwx_test_lang_last: the raw language logits the state's last
        detection pass fed the kernel; empty when it kept none."""
        fn = lib().mwx_test_lang_last
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int]
        out = np.zeros(lang_max_id() + 1, np.float32)
        n = fn(self.state(state_index), fptr(out), out.size)
        self._hook_rc("mwx_test_lang_last", min(n, 0))
        return out[:n]

    # ---- transcript alignment (mwx.h mwx_align_batch) ----
    def align_batch(self, pcms: Sequence[np.ndarray], tokens: Sequence[Sequence[int]],
                    params: FullParams, state_indices: Optional[Sequence[int]] = None,
                    lang_ids=None) -> int:
        """mwx_align_batch: clip b and its text tokens on state state_indices[b]
        (default b). Returns the call's code; segments() / align_rows() read
        the result."""
        n = len(pcms)
        params = self._lang_params(params, lang_ids, n)
        idx = list(range(n)) if state_indices is None else list(state_indices)
        arrs = [np.ascontiguousarray(p, dtype=np.float32) for p in pcms]
        toks = [np.ascontiguousarray(t, dtype=np.int32).reshape(-1) for t in tokens]
        states = (C.c_void_p * n)(*[self.state(i) for i in idx])
        ptrs = (C.POINTER(C.c_float) * n)(*[fptr(a) for a in arrs])
        lens = (C.c_int * n)(*[len(a) for a in arrs])
        ip = C.POINTER(C.c_int32)
        tptr = (ip * n)(*[t.ctypes.data_as(ip) for t in toks])
        tlen = (C.c_int * n)(*[len(t) for t in toks])
        self._keep = (arrs, toks)
        fn = lib().mwx_align_batch
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), FullParams,
                       C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_int), C.POINTER(ip),
                       C.POINTER(C.c_int), C.c_int]
        return fn(self.ctx, states, params, ptrs, lens, tptr, tlen, n)

    def align_rows(self, state_index: int = 0) -> np.ndarray:
        """The rows of the state's last align_batch (mwx_align_row): a record
        array of SCORE_OUT without p, n + 1 rows (the last one: EOT); empty
        when the state has none."""
        fn = lib().mwx_align_row
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int32),
                       C.POINTER(C.c_float)]
        s = self.state(state_index)
        rows = []
        while True:
            plog, top, tplog = C.c_float(), C.c_int32(), C.c_float()
            if fn(s, len(rows), C.byref(plog), C.byref(top), C.byref(tplog)) != 0:
                break
            rows.append((plog.value, top.value, tplog.value))
        return np.array(rows, dtype=[("plog", np.float32), ("top_id", np.int32),
                                     ("top_plog", np.float32)])

    def test_score_rows_rc(self, logits: np.ndarray, target, active):
        """mwx_test_score_rows: logits [R][V] f32, target [R], active [R].
        Returns (rc, plog, p, top_id, top_plog), [R] each; what the launch did
        not write is NaN (top_id: -1)."""
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        R, V = logits.shape
        target = np.ascontiguousarray(target, dtype=np.int32)
        active = np.ascontiguousarray(active, dtype=np.int32)
        assert target.shape == (R,) and active.shape == (R,)
        plog, p, tplog = (np.full(R, np.nan, np.float32) for _ in range(3))
        top = np.full(R, -1, np.int32)
        fn = lib().mwx_test_score_rows
        fpp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, fpp, ip, ip, fpp, fpp, ip, fpp]
        rc = fn(self.ctx, R, V, fptr(logits), target.ctypes.data_as(ip), active.ctypes.data_as(ip),
                fptr(plog), fptr(p), top.ctypes.data_as(ip), fptr(tplog))
        return rc, plog, p, top, tplog

    def test_lang_probs_rc(self, logits: np.ndarray, t0: int, n: int, R: Optional[int] = None,
                           V: Optional[int] = None):
        """mwx_test_lang_probs: logits [R][V] f32, the n entries from t0 of each
        row. Returns (rc, probs [R][n], best [R]); what the call did not write
        is NaN (best: -1). R and V override the array's shape (the refusals)."""
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        aR, aV = logits.shape
        R = aR if R is None else R
        V = aV if V is None else V
        probs = np.full((max(R, 1), min(max(n, 1), 128)), np.nan, np.float32)
        best = np.full(max(R, 1), -1, np.int32)
        fn = lib().mwx_test_lang_probs
        fpp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, fpp, C.c_int, C.c_int, fpp, ip]
        rc = fn(self.ctx, R, V, fptr(logits), t0, n, fptr(probs), best.ctypes.data_as(ip))
        return rc, probs, best

    def test_logits_bias_rc(self, phrases, logits: np.ndarray, hist, active, sample):
        """mwx_test_logits_bias: phrases as (token ids, boost) pairs, logits
        [R][V] f32, hist a list of R id lists, active / sample [R]. Returns
        (rc, logits_out [R][V], state_out [R]); what the call did not write is
        NaN (state: -1)."""
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        R, V = logits.shape
        H = max([len(h) for h in hist] + [1])
        hh = np.zeros((R, H), np.int32)
        hl = np.zeros(R, np.int32)
        for r, h in enumerate(hist):
            hh[r, :len(h)] = h
            hl[r] = len(h)
        active = np.ascontiguousarray(active, dtype=np.int32)
        sample = np.ascontiguousarray(sample, dtype=np.int32)
        assert active.shape == (R,) and sample.shape == (R,) and len(hist) == R
        arr, keep = bias_phrases(phrases)
        out = np.full((R, V), np.nan, np.float32)
        state = np.full(R, -1, np.int32)
        fn = lib().mwx_test_logits_bias
        fpp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(BiasPhrase), C.c_int, C.c_int, C.c_int, fpp, ip,
                       C.c_int, ip, ip, ip, fpp, ip]
        rc = fn(self.ctx, arr, 0 if arr is None else len(arr), R, V, fptr(logits),
                hh.ctypes.data_as(ip), H, hl.ctypes.data_as(ip), active.ctypes.data_as(ip),
                sample.ctypes.data_as(ip), fptr(out), state.ctypes.data_as(ip))
        del keep
        return rc, out, state

    def test_logits_bias(self, phrases, logits, hist, active, sample):
        """As test_logits_bias_rc, raising on a non-zero return."""
        rc, out, state = self.test_logits_bias_rc(phrases, logits, hist, active, sample)
        self._hook_rc("mwx_test_logits_bias", rc)
        return out, state

    def test_lang_probs(self, logits, t0: int, n: int):
        """As test_lang_probs_rc, raising on a non-zero return."""
        rc, probs, best = self.test_lang_probs_rc(logits, t0, n)
        self._hook_rc("mwx_test_lang_probs", rc)
        return probs, best

    def test_score_rows(self, logits, target, active):
        """As test_score_rows_rc, raising on a non-zero return."""
        rc, *res = self.test_score_rows_rc(logits, target, active)
        self._hook_rc("mwx_test_score_rows", rc)
        return tuple(res)

    # ---- per-stage test entry points ----
    def hparam(self, name: str) -> int:
        return getattr(lib(), f"mwx_{name}")(self.ctx)

    def token(self, name: str) -> int:
        """special token id: eot, sot, beg, not, nosp, transcribe, translate"""
        return getattr(lib(), f"mwx_token_{name}")(self.ctx)

    def token_bytes(self, ids) -> List[bytes]:
        """mwx_token_to_str of every id, as bytes."""
        L = lib()
        return [L.mwx_token_to_str(self.ctx, int(t)) or b"" for t in ids]

    def test_mel(self, pcm: np.ndarray, state_index: int = 0) -> np.ndarray:
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        n_mels = self.hparam("n_mels")
        n_len = (len(pcm) + 480000) // 160
        out = np.empty((n_mels, n_len), dtype=np.float32)
        r = lib().mwx_test_mel(self.ctx, self.state(state_index), fptr(pcm), len(pcm), fptr(out),
                               out.size)
        if r != n_len:
            raise RuntimeError(f"mwx_test_mel returned {r}")
        return out

    def prosody_batch(self, pcm: np.ndarray, starts, lens, sample_rate: int = 16000,
                      params: Optional[ProsodyParams] = None, state_index: int = 0):
        """mwx_prosody_batch: prosody of segments [starts[i], starts[i] + lens[i])
        of pcm (a numpy f32 array or a DevicePCM)."""
        st = np.ascontiguousarray(starts, np.int64)
        ln = np.ascontiguousarray(lens, np.int64)
        out = (Prosody * max(1, len(st)))()
        if isinstance(pcm, DevicePCM):
            ptr, n = pcm.ptr, pcm.n
        else:
            a = np.ascontiguousarray(pcm, np.float32)
            ptr, n = fptr(a), len(a)
        p = params if params is not None else lib().mwx_prosody_default_params()
        rc = lib().mwx_prosody_batch(self.ctx, self.state(state_index), ptr, n,
                                     st.ctypes.data_as(C.POINTER(C.c_int64)),
                                     ln.ctypes.data_as(C.POINTER(C.c_int64)), len(st),
                                     sample_rate, C.byref(p), out)
        if rc != 0:
            raise RuntimeError(f"mwx_prosody_batch failed ({rc})")
        return list(out)[:len(st)]

    def resample(self, pcm, src_rate: int, dst_rate: int = 16000, state_index: int = 0):
        """mwx_resample (SttEngine::resample_audio on the GPU): the 16 kHz
        samples, or None where the reference returns an empty buffer (equal
        rates, empty input). `pcm` may be a numpy array or a DevicePCM."""
        L = lib()
        if isinstance(pcm, DevicePCM):
            ptr, n = pcm.ptr, pcm.n
        else:
            a = np.ascontiguousarray(pcm, np.float32)
            ptr, n = a.ctypes.data, len(a)
        cap = L.mwx_resample_max_frames(n, src_rate, dst_rate)
        out = np.empty(max(cap, 1), np.float32)
        r = L.mwx_resample(self.ctx, self.state(state_index), ptr, n, src_rate, dst_rate,
                           out.ctypes.data, cap)
        if r < 0:
            raise RuntimeError(f"mwx_resample failed ({r})")
        return out[:r].copy() if r > 0 else None

    def test_sample_draws(self, probs: np.ndarray, logprobs: np.ndarray, u: np.ndarray,
                          ndraw: np.ndarray, exact: bool = False, reps: int = 1):
        """mwx_test_sample_draws: ids [R][KD] and mean us per launch."""
        pr = np.ascontiguousarray(probs, np.float32)
        lp = np.ascontiguousarray(logprobs, np.float32)
        uu = np.ascontiguousarray(u, np.float64)
        nd = np.ascontiguousarray(ndraw, np.int32)
        R, V = pr.shape
        KD = uu.shape[1]
        ids = np.zeros((R, KD), np.int32)
        us = C.c_double()
        rc = lib().mwx_test_sample_draws(self.ctx, fptr(pr), fptr(lp), R, V,
                                         uu.ctypes.data_as(C.POINTER(C.c_double)),
                                         nd.ctypes.data_as(C.POINTER(C.c_int)), KD, int(exact),
                                         reps, ids.ctypes.data_as(C.POINTER(C.c_int)),
                                         C.byref(us))
        if rc != 0:
            raise RuntimeError(f"mwx_test_sample_draws failed ({rc})")
        return ids, us.value

    def test_gemm_mx(self, a: np.ndarray, w: np.ndarray) -> np.ndarray:
        """c = MX-fp8(bf16(a)) @ MX-fp8(bf16(w))^T on the block-scaled fp8 MFMA."""
        a = np.ascontiguousarray(a, dtype=np.float32)
        w = np.ascontiguousarray(w, dtype=np.float32)
        M, K = a.shape
        N = w.shape[0]
        c = np.empty((M, N), np.float32)
        fn = lib().mwx_test_gemm_mx
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float),
                       C.POINTER(C.c_float), C.POINTER(C.c_float)]
        if fn(self.ctx, M, N, K, fptr(a), fptr(w), fptr(c)) != 0:
            raise RuntimeError("mwx_test_gemm_mx failed")
        return c

    def test_gemm_gelu(self, a: np.ndarray, w: np.ndarray, bias: np.ndarray, bf16: bool,
                       use_table: bool) -> np.ndarray:
        """gelu_ggml(a @ w^T + bias) by the encoder FFN1 GEMM (gemm_big, staged
        GELU epilogue), operands rounded to bf16 / f16; table lookup or tanhf."""
        a = np.ascontiguousarray(a, dtype=np.float32)
        w = np.ascontiguousarray(w, dtype=np.float32)
        bias = np.ascontiguousarray(bias, dtype=np.float32)
        M, K = a.shape
        N = w.shape[0]
        out = np.empty((M, N), np.float32)
        fn = lib().mwx_test_gemm_gelu
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float),
                       C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int,
                       C.POINTER(C.c_float)]
        if fn(self.ctx, M, N, K, fptr(a), fptr(w), fptr(bias), int(bf16), int(use_table),
              fptr(out)) != 0:
            raise RuntimeError("mwx_test_gemm_gelu failed")
        return out

    def test_encode(self, pcm: np.ndarray, seek: int = 0, cross: bool = True,
                    state_index: int = 0):
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        L_a = self.hparam("n_audio_ctx")
        d = self.d
        nl = self.n_text_layer
        enc = np.empty((L_a, d), dtype=np.float32)
        k = np.empty((nl, L_a, d), dtype=np.float32) if cross else None
        v = np.empty((nl, L_a, d), dtype=np.float32) if cross else None
        null = C.POINTER(C.c_float)()
        r = lib().mwx_test_encode(self.ctx, self.state(state_index), fptr(pcm), len(pcm), seek,
                                  fptr(enc),
                                  fptr(k) if cross else null, fptr(v) if cross else null)
        if r != 0:
            raise RuntimeError(f"mwx_test_encode returned {r}")
        return enc, k, v

    def audio_ctx_for(self, n_samples: int, seek: int = 0, audio_ctx: int = 0,
                      fit: bool = False) -> int:
        """mwx_audio_ctx_for: the audio context of the window at `seek` of a
        clip of n_samples samples under FullParams.audio_ctx / audio_ctx_fit."""
        return lib().mwx_audio_ctx_for(self.ctx, int(n_samples), int(seek), int(audio_ctx),
                                       bool(fit))

    def test_encode_ctx(self, pcm: np.ndarray, audio_ctx: int, seek: int = 0,
                        state_index: int = 0):
        """mwx_test_encode_ctx: test_encode at an audio context of audio_ctx
        frames (enc [K][d], k / v [n_text_layer][K][d]); the cross K/V and the
        key count stay in the state for test_decode*."""
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        K, d, nl = int(audio_ctx), self.d, self.n_text_layer
        enc = np.empty((K, d), dtype=np.float32)
        k = np.empty((nl, K, d), dtype=np.float32)
        v = np.empty((nl, K, d), dtype=np.float32)
        r = lib().mwx_test_encode_ctx(self.ctx, self.state(state_index), fptr(pcm), len(pcm), seek,
                                      K, fptr(enc), fptr(k), fptr(v))
        if r != 0:
            raise RuntimeError(f"mwx_test_encode_ctx returned {r}")
        return enc, k, v

    def test_encode_dump(self, pcm: np.ndarray, seek: int = 0, state_index: int = 0):
        """mwx_test_encode_dump: (x [L+1][n_ctx][d] f32 — the residual stream
        after the stem and after each layer, [a0, a1, a2, a3] — per layer the
        four GEMM A operands before MX quantization, as float32 from the
        model's 16-bit type)."""
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        n_ctx, d, L = self.hparam("n_audio_ctx"), self.d, self._hp_from_file()[4]
        x = np.empty((L + 1, n_ctx, d), np.float32)
        a = [np.empty((L, n_ctx, d * (4 if g == 3 else 1)), np.uint16) for g in range(4)]
        ptrs = (C.c_void_p * 4)(*[arr.ctypes.data for arr in a])
        r = lib().mwx_test_encode_dump(self.ctx, self.state(state_index), fptr(pcm), len(pcm), seek,
                                       fptr(x), ptrs)
        if r != 0:
            raise RuntimeError(f"mwx_test_encode_dump returned {r}")
        bf16 = self.hparam("model_wtype") == GGML_BF16
        conv = ((lambda u: (u.astype(np.uint32) << 16).view(np.float32)) if bf16 else
                (lambda u: u.view(np.float16).astype(np.float32)))
        return x, [conv(arr) for arr in a]

    def test_decode(self, tokens: Sequence[int]) -> np.ndarray:
        toks = np.ascontiguousarray(tokens, dtype=np.int32)
        V = self.hparam("n_vocab")
        out = np.empty((len(toks), V), dtype=np.float32)
        r = lib().mwx_test_decode(self.ctx, self.state(), toks.ctypes.data_as(C.POINTER(C.c_int)),
                                  len(toks), fptr(out))
        if r != 0:
            raise RuntimeError(f"mwx_test_decode returned {r}")
        return out

    def decode_counters(self, state_index: int = 0, reset: bool = True):
        """(decode steps launched, prompt positions prefilled) on a state since
        the last reset (mwx_test_decode_counters)."""
        st, pf = C.c_long(), C.c_long()
        lib().mwx_test_decode_counters(self.state(state_index), C.byref(st), C.byref(pf),
                                       1 if reset else 0)
        return st.value, pf.value

    def window_counters(self, state_index: int = 0, reset: bool = True):
        """(clip windows decoded, decode attempts run, clip-steps) on a state
        since the last reset (mwx_test_window_counters); attempts - windows =
        fallbacks; clip-steps = decode steps summed over the clips live in them."""
        w, a, cs = C.c_long(), C.c_long(), C.c_long()
        lib().mwx_test_window_counters(self.state(state_index), C.byref(w), C.byref(a),
                                       C.byref(cs), 1 if reset else 0)
        return w.value, a.value, cs.value

    def runahead_fallbacks(self, state_index: int = 0, reset: bool = True) -> int:
        """Run-ahead attempts redone on the host loop (mwx_test_runahead_fallbacks)."""
        return lib().mwx_test_runahead_fallbacks(self.state(state_index), 1 if reset else 0)

    def test_mx_widen(self, codes: np.ndarray, e8: np.ndarray) -> np.ndarray:
        """mwx_test_mx_widen: e4m3 codes (uint8, groups of 8) widened to f16
        with one E8M0 exponent per group, as the cross-attention kernels do."""
        codes = np.ascontiguousarray(codes, np.uint8)
        e8 = np.ascontiguousarray(e8, np.uint8)
        assert codes.size == 8 * e8.size
        out = np.empty(codes.size, np.uint16)
        r = lib().mwx_test_mx_widen(self.ctx, codes.ctypes.data, e8.ctypes.data, e8.size,
                                    out.ctypes.data)
        if r != 0:
            raise RuntimeError(f"mwx_test_mx_widen returned {r}")
        return out.view(np.float16)

    def test_xattn_mx(self, q: np.ndarray, k8: np.ndarray, ks: np.ndarray, v8: np.ndarray,
                      vs: np.ndarray, nq: int) -> np.ndarray:
        """mwx_test_xattn_mx: q [R][H*64] f32; k8 / v8 uint8 [R/nq][H][n][64];
        ks / vs uint8 [R/nq][H][n][2]. Returns o [R][H*64] f32."""
        R, D = q.shape
        G, H, n, _ = k8.shape
        assert G * nq == R and H * 64 == D
        q = np.ascontiguousarray(q, dtype=np.float32)
        arrs = [np.ascontiguousarray(a, dtype=np.uint8) for a in (k8, ks, v8, vs)]
        o = np.empty((R, D), dtype=np.float32)
        u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
        rc = lib().mwx_test_xattn_mx(self.ctx, R, H, n, nq, q.ctypes.data_as(C.POINTER(C.c_float)),
                                     *[u8(a) for a in arrs], o.ctypes.data_as(C.POINTER(C.c_float)))
        if rc != 0:
            raise RuntimeError(f"mwx_test_xattn_mx failed ({rc})")
        return o

    def test_dec_attn(self, P: np.ndarray, bias: np.ndarray, kcache: np.ndarray,
                      vcache: np.ndarray, *, bf16: bool, active, pos=None, kv_index=None,
                      fixed_len: int = 0, qscale: float = 1.0, kscale: float = 1.0,
                      scale: float = 1.0, nq: int = 1, grouped: bool = False,
                      prefill: bool = False, kvmap=None, own_from=None, map_row0: int = 0):
        """mwx_test_dec_attn: one decode attention launch. P [KS][R][pcols] f32,
        kcache / vcache [slots][H][cap][64] float16 (not modified). Returns
        (o [R][H*64] f32, kcache after, vcache after); a row the launch did not
        write is NaN in o. Raises ValueError when the hook refuses the indices."""
        P = np.ascontiguousarray(P, dtype=np.float32)
        bias = np.ascontiguousarray(bias, dtype=np.float32)
        KS, R, pcols = P.shape
        slots, H, cap, _ = kcache.shape
        assert kcache.dtype == np.float16 and vcache.dtype == np.float16
        assert vcache.shape == kcache.shape and kcache.shape[3] == 64
        assert pcols == (H * 64 if fixed_len else 3 * H * 64) and bias.shape == (pcols,)
        kc = np.array(kcache, dtype=np.float16, order="C").view(np.uint16)
        vc = np.array(vcache, dtype=np.float16, order="C").view(np.uint16)
        ip = C.POINTER(C.c_int)

        def ints(a, shape):
            if a is None:
                return None, ip()
            a = np.ascontiguousarray(a, dtype=np.int32)
            assert a.shape == shape, (a.shape, shape)
            return a, a.ctypes.data_as(ip)

        keep = [ints(active, (R,)), ints(pos, (R,)), ints(kv_index, (R,)),
                ints(kvmap, (R, cap)), ints(own_from, (R,))]
        o = np.empty((R, H * 64), np.float32)
        u16 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint16))
        rc = lib().mwx_test_dec_attn(self.ctx, int(bf16), int(grouped), int(prefill), R, H, cap,
                                     slots, KS, nq, fixed_len, fptr(P), fptr(bias), qscale, kscale,
                                     scale, u16(kc), u16(vc), keep[2][1], keep[1][1], keep[0][1],
                                     keep[3][1], keep[4][1], map_row0, fptr(o))
        if rc == -1:
            raise ValueError("mwx_test_dec_attn refused its arguments")
        if rc != 0:
            raise RuntimeError(f"mwx_test_dec_attn failed ({rc})")
        return o, kc.view(np.float16), vc.view(np.float16)

    def test_align_probs(self, P: np.ndarray, bias: np.ndarray, k: np.ndarray, *, heads, A: int,
                         kv_index, pos, active, out: np.ndarray, pos0: int = 0,
                         qscale: float = 1.0, scale: float = 1.0, kscale=None) -> np.ndarray:
        """mwx_test_align_probs: P [KS][R][H*64] f32, bias [H*64], k
        [slots][H][n_keys][64] float16 (or uint8 e4m3 codes with kscale
        [slots][H][n_keys][2] uint8), heads [(head, a), ...], out
        [slots][A][n_rows_cap][n_keys] f32 (a copy is filled and returned; rows
        the launch does not write keep their values)."""
        P = np.ascontiguousarray(P, dtype=np.float32)
        bias = np.ascontiguousarray(bias, dtype=np.float32)
        KS, R, D = P.shape
        slots, H, n_keys, _ = k.shape
        mx = kscale is not None
        assert k.shape[3] == 64 and D == H * 64 and bias.shape == (D,)
        assert k.dtype == (np.uint8 if mx else np.float16)
        kc = np.ascontiguousarray(k)
        ksc = np.ascontiguousarray(kscale, dtype=np.uint8) if mx else None
        assert not mx or ksc.shape == (slots, H, n_keys, 2)
        o = np.array(out, dtype=np.float32, order="C")
        assert o.shape[0] == slots and o.shape[1] == A and o.shape[3] == n_keys
        ip = C.POINTER(C.c_int)
        hd = np.ascontiguousarray(heads, dtype=np.int32).reshape(-1, 2)
        ints = [np.ascontiguousarray(a, dtype=np.int32) for a in (kv_index, pos, active)]
        assert all(a.shape == (R,) for a in ints)
        fn = lib().mwx_test_align_probs
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p] + [C.c_int] * 7 + [ip, C.c_int, C.c_int, C.c_int,
                                                      C.POINTER(C.c_float), C.POINTER(C.c_float),
                                                      C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                                                      ip, ip, ip, C.POINTER(C.c_float)]
        rc = fn(self.ctx, int(mx), R, H, KS, n_keys, slots, len(hd), hd.ctypes.data_as(ip), A, pos0,
                o.shape[2], fptr(P), fptr(bias), qscale, scale, kc.ctypes.data,
                ksc.ctypes.data if mx else None, *[a.ctypes.data_as(ip) for a in ints], fptr(o))
        if rc == -1:
            raise ValueError("mwx_test_align_probs refused its arguments")
        if rc != 0:
            raise RuntimeError(f"mwx_test_align_probs failed ({rc})")
        return o

    def test_dtw_cost(self, w: np.ndarray, Ns, Ts) -> List[np.ndarray]:
        """mwx_test_dtw_cost: w [B][A][n_rows_cap][n_keys] f32 probabilities;
        returns clip b's cost matrix [Ns[b]][Ts[b]]."""
        w = np.ascontiguousarray(w, dtype=np.float32)
        B, A, ncap, n_keys = w.shape
        ns = np.ascontiguousarray(Ns, dtype=np.int32)
        ts = np.ascontiguousarray(Ts, dtype=np.int32)
        assert ns.shape == (B,) and ts.shape == (B,)
        stride = ncap * int(ts.max())
        cost = np.empty(B * stride, np.float32)
        ip = C.POINTER(C.c_int)
        fn = lib().mwx_test_dtw_cost
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p] + [C.c_int] * 4 + [ip, ip, C.POINTER(C.c_float),
                                                      C.POINTER(C.c_float)]
        rc = fn(self.ctx, B, A, ncap, n_keys, ns.ctypes.data_as(ip), ts.ctypes.data_as(ip), fptr(w),
                fptr(cost))
        if rc != 0:
            raise RuntimeError(f"mwx_test_dtw_cost failed ({rc})")
        return [cost[b * stride:b * stride + ns[b] * ts[b]].reshape(ns[b], ts[b]).copy()
                for b in range(B)]

    def test_dtw_path(self, costs: Sequence[np.ndarray]):
        """mwx_test_dtw_path: the DTW of B cost matrices [N_b][T_b] in one
        launch. Returns [(frames [N_b], path [L_b][2] (row, column)), ...]."""
        B = len(costs)
        ns = np.array([c.shape[0] for c in costs], np.int32)
        ts = np.array([c.shape[1] for c in costs], np.int32)
        nm, tm = int(ns.max()), int(ts.max())
        flat = np.zeros(B * nm * tm, np.float32)
        for b, c in enumerate(costs):
            flat[b * nm * tm:b * nm * tm + c.size] = np.ascontiguousarray(c, np.float32).ravel()
        frames = np.empty((B, nm), np.int32)
        path = np.empty((B, nm + tm, 2), np.int32)
        plen = np.empty(B, np.int32)
        ip = C.POINTER(C.c_int)
        fn = lib().mwx_test_dtw_path
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int, ip, ip, C.POINTER(C.c_float), ip, ip, ip]
        rc = fn(self.ctx, B, ns.ctypes.data_as(ip), ts.ctypes.data_as(ip), fptr(flat),
                frames.ctypes.data_as(ip), path.ctypes.data_as(ip), plen.ctypes.data_as(ip))
        if rc != 0:
            raise RuntimeError(f"mwx_test_dtw_path failed ({rc})")
        return [(frames[b, :ns[b]].copy(), path[b, nm + tm - plen[b]:].copy()) for b in range(B)]

    def dtw_keep(self, on: bool = True, state_index: int = 0) -> None:
        """mwx_test_dtw_keep: the state keeps its DTW passes for dtw_passes()."""
        fn = lib().mwx_test_dtw_keep
        fn.argtypes = [C.c_void_p, C.c_int]
        fn(self.state(state_index), int(on))

    def test_dtw_align(self, tokens, pos0: int, n_cols: int, state_index: int = 0) -> dict:
        """mwx_test_dtw_align: the alignment pass over `tokens` against the
        cross K/V of the last test_encode on the state; returns the pass."""
        tk = np.ascontiguousarray(tokens, dtype=np.int32)
        fn = lib().mwx_test_dtw_align
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int]
        rc = fn(self.ctx, self.state(state_index), tk.ctypes.data_as(C.POINTER(C.c_int)), len(tk),
                pos0, n_cols)
        if rc != 0:
            raise RuntimeError(f"mwx_test_dtw_align failed ({rc})")
        return self.dtw_passes(state_index)[0]

    def dtw_passes(self, state_index: int = 0) -> List[dict]:
        """The DTW passes (one per window that emitted segments) of the
        state's last call: dicts with seek, probs [A][N][n_audio_ctx], cost
        [N][T], frames [N]."""
        L = lib()
        L.mwx_test_dtw_n_passes.argtypes = [C.c_void_p]
        fn = L.mwx_test_dtw_last
        fn.restype = C.c_int
        ip = C.POINTER(C.c_int)
        fn.argtypes = [C.c_void_p, C.c_int, ip, C.POINTER(C.c_int64), C.POINTER(C.c_float),
                       C.c_long, C.POINTER(C.c_float), C.c_long, ip, C.c_long]
        s = self.state(state_index)
        out = []
        for i in range(max(0, L.mwx_test_dtw_n_passes(s))):
            dims = (C.c_int * 4)()
            seek = C.c_int64()
            if fn(s, i, dims, C.byref(seek), None, 0, None, 0, None, 0) != 0:
                raise RuntimeError("mwx_test_dtw_last failed")
            N, T, A, nk = list(dims)
            probs = np.empty((A, N, nk), np.float32)
            cost = np.empty((N, T), np.float32)
            frames = np.empty(N, np.int32)
            if fn(s, i, dims, C.byref(seek), fptr(probs), probs.size, fptr(cost), cost.size,
                  frames.ctypes.data_as(ip), N) != 0:
                raise RuntimeError("mwx_test_dtw_last failed")
            out.append(dict(seek=seek.value, probs=probs, cost=cost, frames=frames))
        return out

    def test_gemm_dec(self, a: np.ndarray, w: np.ndarray, *, bf16: bool, mode: int,
                      bias=None, res=None) -> np.ndarray:
        """mwx_test_gemm_dec: a [M][K], w [N][K] f32 (rounded to bf16 / f16 by the
        hook). mode 0: the split-K slabs [KS][M][N]; mode 1: c [M][N] (EPI_F32);
        mode 2: (a.w + bias) + res (EPI_RES)."""
        a = np.ascontiguousarray(a, dtype=np.float32)
        w = np.ascontiguousarray(w, dtype=np.float32)
        M, K = a.shape
        N = w.shape[0]
        assert w.shape == (N, K)
        null = C.POINTER(C.c_float)()
        if bias is not None:
            bias = np.ascontiguousarray(bias, dtype=np.float32)
            assert bias.shape == (N,)
        if res is not None:
            res = np.ascontiguousarray(res, dtype=np.float32)
            assert res.shape == (M, N)
        out = np.empty((8 if mode == 0 else 1, M, N), np.float32)
        ks = C.c_int(0)
        rc = lib().mwx_test_gemm_dec(self.ctx, int(bf16), mode, M, N, K, fptr(a), fptr(w),
                                     null if bias is None else fptr(bias),
                                     null if res is None else fptr(res), C.byref(ks), fptr(out))
        if rc == -1:
            raise ValueError("mwx_test_gemm_dec refused its arguments")
        if rc != 0:
            raise RuntimeError(f"mwx_test_gemm_dec failed ({rc})")
        return out[:ks.value].copy() if mode == 0 else out[0]

    def test_gemm_dec_ex(self, a=None, w=None, *, bf16: bool, mode: int, wq=None, ws=None,
                         bias=None, res=None, ln=None):
        """mwx_test_gemm_dec_ex (include/mwx_test.h). a [M][K] f32; the weights
        as w [N][K] f32 or as MX-fp8 codes wq [N][K] and scales ws [N][K/32]
        (uint8; either selects w8). ln: a dict x_in [K], w, b [K], active
        (0 / 1), P [KS][K] and pbias [K] (or neither): the folded LayerNorm
        as the A operand (M = 1). Returns the slabs [KS][M][N] (mode 0), c
        [M][N] (modes 1, 2) or (c [M][N], the packed buffer's uint16 words
        [ceil64(M)][N] flat) (mode 3); with ln, a tuple of that, x_out (the
        uint32 words of the residual buffer) and x_in as read back."""
        f32 = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float32)
        u8 = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.uint8)
        a, w, bias, res, wq, ws = f32(a), f32(w), f32(bias), f32(res), u8(wq), u8(ws)
        g = TestGemmDecArgs()
        g.bf16, g.mode = int(bf16), mode
        g.w8 = int(wq is not None or ws is not None)
        g.ln = int(ln is not None)
        x_in = x_out = None
        keep = []
        ptr = lambda x, t: C.POINTER(t)() if x is None else x.ctypes.data_as(C.POINTER(t))
        if ln is not None:
            x_in = np.array(ln["x_in"], dtype=np.float32, order="C")
            K = x_in.shape[0]
            x_out = np.empty(K, np.uint32)
            P, pbias = f32(ln.get("P")), f32(ln.get("pbias"))
            lw, lb = f32(ln["w"]), f32(ln["b"])
            act = np.asarray([ln.get("active", 1)], np.int32)
            assert x_in.shape == lw.shape == lb.shape == (K,)
            g.KS = 0 if P is None else P.shape[0]
            assert P is None or P.shape == (g.KS, K)
            assert pbias is None or pbias.shape == (K,)
            keep += [P, pbias, lw, lb, act]
            g.x_in, g.x_out = ptr(x_in, C.c_float), ptr(x_out.view(np.float32), C.c_float)
            g.P, g.pbias = ptr(P, C.c_float), ptr(pbias, C.c_float)
            g.ln_w, g.ln_b, g.active = ptr(lw, C.c_float), ptr(lb, C.c_float), ptr(act, C.c_int)
        M = 1 if a is None else a.shape[0]
        N = next(x.shape[0] for x in (w, wq, ws, bias) if x is not None)
        K = next(x.shape[-1] for x in (a, x_in, w, wq) if x is not None)
        for x in (w, wq):
            assert x is None or x.shape == (N, K), x.shape
        assert ws is None or ws.shape == (N, K // 32), ws.shape
        assert bias is None or bias.shape == (N,)
        assert res is None or res.shape == (M, N)
        g.M, g.N, g.K = M, N, K
        g.a, g.w, g.bias, g.res = (ptr(x, C.c_float) for x in (a, w, bias, res))
        g.wq, g.ws = ptr(wq, C.c_uint8), ptr(ws, C.c_uint8)
        out = np.empty((8 if mode == 0 else 1, M, N), np.float32)
        out16 = np.empty((M + 63) // 64 * 64 * N, np.uint16) if mode == 3 else None
        ks = C.c_int(0)
        g.ks_out, g.out, g.out16 = C.pointer(ks), ptr(out, C.c_float), ptr(out16, C.c_uint16)
        fn = lib().mwx_test_gemm_dec_ex
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(TestGemmDecArgs)]
        self._hook_rc("mwx_test_gemm_dec_ex", fn(self.ctx, C.byref(g)))
        got = out[:ks.value].copy() if mode == 0 else (out[0], out16) if mode == 3 else out[0]
        return got if ln is None else (got, x_out, x_in)

    @staticmethod
    def _hook_rc(name: str, rc: int):
        if rc == -1:
            raise ValueError(f"{name} refused its arguments")
        if rc == -4:
            raise NotImplementedError(f"{name}: shape not served by the kernel family")
        if rc != 0:
            raise RuntimeError(f"{name} failed ({rc})")

    def test_enc_attn(self, q: np.ndarray, k: np.ndarray, vt: np.ndarray, *, bf16: bool,
                      scale: float, lens=None) -> np.ndarray:
        """mwx_test_enc_attn: q, k [B][H][L][64] and vt [B][H][64][Lp] float16
        (Lp = L rounded up to 8, pad columns included). Returns o [B*L][H*64]
        f32; a word the launch did not write is NaN."""
        assert q.dtype == np.float16 and k.dtype == np.float16 and vt.dtype == np.float16
        B, H, L, _ = q.shape
        assert q.shape == (B, H, L, 64) and k.shape == q.shape
        assert vt.shape == (B, H, 64, (L + 7) & ~7), vt.shape
        q, k, vt = (np.ascontiguousarray(a).view(np.uint16) for a in (q, k, vt))
        ip, u16p = C.POINTER(C.c_int), C.POINTER(C.c_uint16)
        if lens is not None:
            lens = np.ascontiguousarray(lens, dtype=np.int32)
            assert lens.shape == (B,)
        o = np.empty((B * L, H * 64), np.float32)
        fn = lib().mwx_test_enc_attn
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p] + [C.c_int] * 4 + [ip, C.c_float, u16p, u16p, u16p,
                                                      C.POINTER(C.c_float)]
        rc = fn(self.ctx, int(bf16), B, H, L, ip() if lens is None else lens.ctypes.data_as(ip),
                scale, q.ctypes.data_as(u16p), k.ctypes.data_as(u16p), vt.ctypes.data_as(u16p),
                fptr(o))
        self._hook_rc("mwx_test_enc_attn", rc)
        return o

    def test_gemm_enc(self, epi: int, a: np.ndarray, w: np.ndarray, *, bf16: bool, M: int,
                      lda: Optional[int] = None, a_bstride: int = 0, batch: int = 1, bias=None,
                      pe=None, c16=None, c32=None, ldc: Optional[int] = None, c_bstride: int = 0,
                      c_off: int = 0, out16: bool = False, use_table: bool = True, L: int = 0,
                      H: int = 0, d: int = 0, ldv: int = 0, lcap: int = 0, ncap: int = 0,
                      slot=None, kscale: float = 1.0, q=None, k=None, v=None, mx: bool = False,
                      kv8=None):
        """mwx_test_gemm_enc (include/mwx_test.h): a = any f32 array (read flat
        through lda / a_bstride), w [N][K]. The output arrays (c16 uint16 / c32
        float32 flat, q / k / v uint16) are copied, run through the launch and
        returned: c16 | c32 | (q, k, v) | (k, v). kv8 = (k8, v8, ks8, vs8) uint8:
        the MX-fp8 cross cache instead of k / v, returned as such a tuple."""
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
        w = np.ascontiguousarray(w, dtype=np.float32)
        N, K = w.shape
        f32 = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float32)
        u16 = lambda x: None if x is None else np.array(x, dtype=np.uint16, order="C")
        bias, pe = f32(bias), f32(pe)
        c16, q, k, v = u16(c16), u16(q), u16(k), u16(v)
        c32 = None if c32 is None else np.array(c32, dtype=np.float32, order="C")
        slot = None if slot is None else np.ascontiguousarray(slot, dtype=np.int32)
        g = TestGemmEncArgs()
        g.bf16, g.epi, g.out16, g.use_table = int(bf16), epi, int(out16), int(use_table)
        g.mx, g.kv8 = int(mx), int(kv8 is not None)
        if kv8 is not None:
            kv8 = tuple(np.array(x, dtype=np.uint8, order="C") for x in kv8)
            assert d > 0 and kv8[0].size == kv8[1].size == (N // (2 * d)) * ncap * H * lcap * 64
            assert kv8[2].size == kv8[3].size == kv8[0].size // 32
            g.k8, g.v8, g.ks8, g.vs8 = (x.ctypes.data_as(C.POINTER(C.c_uint8)) for x in kv8)
        g.M, g.N, g.K, g.batch = M, N, K, batch
        g.lda, g.a_bstride, g.a_len = K if lda is None else lda, a_bstride, a.size
        cbuf = c16 if c16 is not None else c32
        g.ldc, g.c_bstride, g.c_off = N if ldc is None else ldc, c_bstride, c_off
        g.c_len = 0 if cbuf is None else cbuf.size
        g.L, g.H, g.d, g.ldv, g.lcap, g.ncap, g.kscale = L, H, d, ldv, lcap, ncap, kscale
        if pe is not None:
            assert pe.shape == (M, g.ldc), pe.shape
        if bias is not None:
            assert bias.shape == (N,)
        if slot is not None:
            assert L > 0 and slot.shape == (M // L,)
        if epi == EPI_ENC_QKV and L > 0 and H > 0 and ldv > 0 and q is not None:
            assert q.size == k.size == (M // L) * H * L * 64 and v.size == (M // L) * H * 64 * ldv
        if epi == EPI_CROSS_KV and d > 0 and k is not None:
            assert k.size == v.size == (N // (2 * d)) * ncap * H * lcap * 64
        ptr = lambda x, t: C.POINTER(t)() if x is None else x.ctypes.data_as(C.POINTER(t))
        g.a, g.w = ptr(a, C.c_float), ptr(w, C.c_float)
        g.bias, g.pe, g.slot = ptr(bias, C.c_float), ptr(pe, C.c_float), ptr(slot, C.c_int)
        g.c16, g.c32 = ptr(c16, C.c_uint16), ptr(c32, C.c_float)
        g.q, g.k, g.v = ptr(q, C.c_uint16), ptr(k, C.c_uint16), ptr(v, C.c_uint16)
        fn = lib().mwx_test_gemm_enc
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(TestGemmEncArgs)]
        self._hook_rc("mwx_test_gemm_enc", fn(self.ctx, C.byref(g)))
        if epi == EPI_GELU:
            return c16
        if epi in (EPI_RES, EPI_CONV2):
            return c32
        if kv8 is not None:
            return kv8
        return (q, k, v) if epi == EPI_ENC_QKV else (k, v)

    def test_layer_norm(self, x: np.ndarray, w: np.ndarray, b: np.ndarray, *, bf16: bool,
                        dec: bool = False, active=None, P=None, pbias=None, te=None, pe=None,
                        tok=None, pos=None):
        """mwx_test_layer_norm: x [M][N] f32 (not modified). Returns (y [M][N]
        f32, x after the launch); a row the launch did not write is NaN in y."""
        x = np.array(x, dtype=np.float32, order="C")
        M, N = x.shape
        f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
        i32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)
        w, b, P, pbias, te, pe = (f32(a) for a in (w, b, P, pbias, te, pe))
        active, tok, pos = (i32(a) for a in (active, tok, pos))
        assert w.shape == (N,) and b.shape == (N,)
        KS = 0
        if P is not None:
            KS = P.shape[0]
            assert P.shape == (KS, M, N) and pbias.shape == (N,)
        for a in (active, tok, pos):
            assert a is None or a.shape == (M,)
        n_tok = n_pos = 0
        if te is not None:
            n_tok, n_pos = te.shape[0], pe.shape[0]
            assert te.shape == (n_tok, N) and pe.shape == (n_pos, N)
        fpp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
        fp = lambda a: fpp() if a is None else fptr(a)
        ipt = lambda a: ip() if a is None else a.ctypes.data_as(ip)
        y = np.empty((M, N), np.float32)
        fn = lib().mwx_test_layer_norm
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p] + [C.c_int] * 4 + [fpp, fpp, fpp, ip, fpp, C.c_int, fpp, fpp,
                                                      fpp, ip, ip, C.c_int, C.c_int, fpp]
        rc = fn(self.ctx, int(bf16), int(dec), M, N, fptr(x), fptr(w), fptr(b), ipt(active), fp(P),
                KS, fp(pbias), fp(te), fp(pe), ipt(tok), ipt(pos), n_tok, n_pos, fptr(y))
        self._hook_rc("mwx_test_layer_norm", rc)
        return y, x

    def test_logits_process_rc(self, logits: np.ndarray, smask: np.ndarray, ctl: np.ndarray,
                               lc: TestLogitsConst):
        """mwx_test_logits_process: logits [R][V] f32, smask [V], ctl [R] of
        LOGITS_CTL, lc. Returns (rc, flt, probs, logprobs [R][V], out [R] of
        LOGITS_OUT); whatever the launch did not write is NaN (id, tid: -1)."""
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        smask = np.ascontiguousarray(smask, dtype=np.float32)
        ctl = np.ascontiguousarray(ctl, dtype=LOGITS_CTL)
        R, V = logits.shape
        assert smask.shape == (V,) and ctl.shape == (R,)
        flt, probs, logprobs = (np.full((R, V), np.nan, np.float32) for _ in range(3))
        out = np.zeros(R, LOGITS_OUT)
        out.view(np.uint32)[:] = 0xFFFFFFFF
        fn = lib().mwx_test_logits_process
        fpp = C.POINTER(C.c_float)
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, fpp, fpp, C.c_void_p,
                       C.POINTER(TestLogitsConst), fpp, fpp, fpp, C.c_void_p]
        rc = fn(self.ctx, R, V, fptr(logits), fptr(smask), ctl.ctypes.data, C.byref(lc),
                fptr(flt), fptr(probs), fptr(logprobs), out.ctypes.data)
        return rc, flt, probs, logprobs, out

    def test_logits_process_masked_rc(self, logits: np.ndarray, smask: np.ndarray,
                                      ctl: np.ndarray, lc: TestLogitsConst, cmask: np.ndarray,
                                      penalty: float):
        """mwx_test_logits_process_masked: as test_logits_process_rc with the
        filter's rejection words cmask [R][ceil(V / 64)] uint64 and the penalty."""
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        smask = np.ascontiguousarray(smask, dtype=np.float32)
        ctl = np.ascontiguousarray(ctl, dtype=LOGITS_CTL)
        cmask = np.ascontiguousarray(cmask, dtype=np.uint64)
        R, V = logits.shape
        assert smask.shape == (V,) and ctl.shape == (R,) and cmask.shape == (R, (V + 63) // 64)
        flt, probs, logprobs = (np.full((R, V), np.nan, np.float32) for _ in range(3))
        out = np.zeros(R, LOGITS_OUT)
        out.view(np.uint32)[:] = 0xFFFFFFFF
        fn = lib().mwx_test_logits_process_masked
        fpp = C.POINTER(C.c_float)
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, fpp, fpp, C.c_void_p,
                       C.POINTER(TestLogitsConst), C.c_void_p, C.c_float, fpp, fpp, fpp,
                       C.c_void_p]
        rc = fn(self.ctx, R, V, fptr(logits), fptr(smask), ctl.ctypes.data, C.byref(lc),
                cmask.ctypes.data, float(penalty), fptr(flt), fptr(probs), fptr(logprobs),
                out.ctypes.data)
        return rc, flt, probs, logprobs, out

    def test_constraint_mask_rc(self, constraint: "Constraint", states, active, sample,
                                V=None, eot: int = 0, tokens=None):
        """mwx_test_constraint_mask: one logits_constrain launch on R rows in the
        given constraint states. tokens: None (the context's vocabulary; V its
        n_vocab) or a list of the byte strings of the ids below eot = len(tokens)
        (then V must be given). Returns (rc, mask [R][ceil(V / 64)] uint64); a
        word the launch did not write is all ones."""
        states = np.ascontiguousarray(states, dtype=np.int32)
        active = np.ascontiguousarray(active, dtype=np.int32)
        sample = np.ascontiguousarray(sample, dtype=np.int32)
        R = len(states)
        assert active.shape == (R,) and sample.shape == (R,)
        u32, u8, ip = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
        if tokens is None:
            V = self.hparam("n_vocab") if V is None else V
            offp, bytp, eot = u32(), u8(), 0
            keep = None
        else:
            eot = len(tokens)
            off = np.zeros(eot + 1, np.uint32)
            off[1:] = np.cumsum([len(t) for t in tokens], dtype=np.uint64)
            data = np.frombuffer(b"".join(tokens) + b"\0", dtype=np.uint8)
            offp, bytp, keep = off.ctypes.data_as(u32), data.ctypes.data_as(u8), (off, data)
        W = (max(V, 1) + 63) // 64
        mask = np.full((max(R, 1), W), 0xFFFFFFFFFFFFFFFF, np.uint64)
        fn = lib().mwx_test_constraint_mask
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, u32, u8, ip, ip, ip,
                       C.c_void_p]
        rc = fn(self.ctx, None if constraint is None else constraint.ptr, R, V, eot, offp, bytp,
                states.ctypes.data_as(ip), active.ctypes.data_as(ip), sample.ctypes.data_as(ip),
                mask.ctypes.data)
        del keep
        return rc, mask

    def constraint_status(self, state_index: int = 0) -> int:
        """mwx_full_constraint_status_from_state."""
        fn = lib().mwx_full_constraint_status_from_state
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p]
        return fn(self.state(state_index))

    def test_logits_process(self, logits, smask, ctl, lc):
        """As test_logits_process_rc, raising on a non-zero return."""
        rc, *res = self.test_logits_process_rc(logits, smask, ctl, lc)
        self._hook_rc("mwx_test_logits_process", rc)
        return tuple(res)

    def test_logits_setup(self, params: FullParams):
        """mwx_test_logits_setup: the engine's (LogitsConst, static mask [V]) for
        a call with `params`."""
        lc = TestLogitsConst()
        smask = np.empty(self.hparam("n_vocab"), np.float32)
        fn = lib().mwx_test_logits_setup
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(FullParams), C.POINTER(TestLogitsConst),
                       C.POINTER(C.c_float)]
        self._hook_rc("mwx_test_logits_setup", fn(self.ctx, C.byref(params), C.byref(lc),
                                                  fptr(smask)))
        return lc, smask

    def test_gelu_table(self) -> np.ndarray:
        """The device-built f16 GELU table as uint16 bits (index: see
        mwx_test_gelu_table)."""
        L = lib()
        L.mwx_test_gelu_table_size.restype = C.c_int
        L.mwx_test_gelu_table_size.argtypes = []
        tab = np.empty(L.mwx_test_gelu_table_size(), np.uint16)
        L.mwx_test_gelu_table.restype = C.c_int
        L.mwx_test_gelu_table.argtypes = [C.c_void_p, C.POINTER(C.c_uint16)]
        self._hook_rc("mwx_test_gelu_table",
                      L.mwx_test_gelu_table(self.ctx, tab.ctypes.data_as(C.POINTER(C.c_uint16))))
        return tab

    def test_decode_last(self, tokens: Sequence[int], out: Optional[np.ndarray] = None,
                         state_index: int = 0) -> np.ndarray:
        toks = np.ascontiguousarray(tokens, dtype=np.int32)
        if out is None:
            out = np.empty(self.hparam("n_vocab"), dtype=np.float32)
        r = lib().mwx_test_decode_last(self.ctx, self.state(state_index),
                                       toks.ctypes.data_as(C.POINTER(C.c_int)), len(toks), fptr(out))
        if r != 0:
            raise RuntimeError(f"mwx_test_decode_last returned {r}")
        return out

    def test_self_kv(self, layer: int, n_pos: int, state_index: int = 0):
        """(K, V) of row 0's self-attention cache, layer `layer`, positions < n_pos."""
        H = self.d // 64
        k = np.empty((n_pos, H, 64), np.float32)
        v = np.empty_like(k)
        r = lib().mwx_test_self_kv(self.state(state_index), layer, n_pos, fptr(k), fptr(v))
        if r != 0:
            raise RuntimeError(f"mwx_test_self_kv returned {r}")
        return k, v

    def test_decode_last_prefill(self, tokens: Sequence[int], state_index: int = 0) -> np.ndarray:
        """test_decode_last with tokens[:-1] through the batched prompt prefill."""
        toks = np.ascontiguousarray(tokens, dtype=np.int32)
        out = np.empty(self.hparam("n_vocab"), dtype=np.float32)
        r = lib().mwx_test_decode_last_prefill(self.ctx, self.state(state_index),
                                               toks.ctypes.data_as(C.POINTER(C.c_int)), len(toks),
                                               fptr(out))
        if r != 0:
            raise RuntimeError(f"mwx_test_decode_last_prefill returned {r}")
        return out

    @property
    def d(self) -> int:
        return self._hp_from_file()[2]

    @property
    def n_text_layer(self) -> int:
        return self._hp_from_file()[8]

    def _hp_from_file(self):
        if not hasattr(self, "_hp"):
            raise RuntimeError("hparams unknown: use Context.open()")
        return self._hp

    @classmethod
    def open(cls, model_path: str, device: int = 0, compute: int = COMPUTE_MODEL,
             **dtw) -> "Context":
        c = cls(model_path, device, compute, **dtw)
        c._hp = read_hparams(model_path)
        return c


class VadContext:
    """mwx_vad_context: one speech probability per 512-sample chunk of 16 kHz
    f32 PCM. Clips may be numpy arrays or DevicePCM buffers (Context.upload) of
    the same GPU. One call at a time per context."""

    def __init__(self, model_path: str, device: int = 0):
        L = lib()
        vp = L.mwx_vad_default_context_params()
        vp.gpu_device = device
        self.vctx = L.mwx_vad_init_from_file_with_params(model_path.encode(), vp)
        if not self.vctx:
            raise RuntimeError(f"mwx_vad_init_from_file_with_params failed for {model_path}")

    def close(self):
        if self.vctx:
            lib().mwx_vad_free(self.vctx)
            self.vctx = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @staticmethod
    def _clip(pcm):
        """(keep-alive object, address, sample count)"""
        if isinstance(pcm, DevicePCM):
            return pcm, C.cast(pcm.ptr, C.c_void_p).value, pcm.n
        a = np.ascontiguousarray(pcm, dtype=np.float32)
        return a, a.ctypes.data, len(a)

    def detect(self, pcm) -> np.ndarray:
        """mwx_vad_detect_speech + mwx_vad_probs: the chunk probabilities."""
        L = lib()
        _keep, addr, n = self._clip(pcm)
        if not L.mwx_vad_detect_speech(self.vctx, addr, n):
            raise RuntimeError("mwx_vad_detect_speech failed")
        k = L.mwx_vad_n_probs(self.vctx)
        if k == 0:
            return np.empty(0, np.float32)
        return np.ctypeslib.as_array(L.mwx_vad_probs(self.vctx), shape=(k,)).copy()

    def detect_batch(self, pcms) -> List[np.ndarray]:
        """mwx_vad_detect_speech_batch: every clip in one pass."""
        L = lib()
        clips = [self._clip(p) for p in pcms]
        n = len(clips)
        if n == 0:
            return []
        counts = [L.mwx_vad_n_chunks(c[2]) for c in clips]
        offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        out = np.empty(max(1, int(offs[-1])), np.float32)
        ptrs = (C.c_void_p * n)(*[c[1] for c in clips])
        lens = (C.c_int * n)(*[c[2] for c in clips])
        rc = L.mwx_vad_detect_speech_batch(self.vctx, ptrs, lens, n, fptr(out),
                                           offs.ctypes.data_as(C.POINTER(C.c_int)))
        if rc != 0:
            raise RuntimeError(f"mwx_vad_detect_speech_batch failed ({rc})")
        return [out[offs[i]:offs[i + 1]].copy() for i in range(n)]

    def last_kernel_ms(self):
        """(front end, recurrence + head) device milliseconds of the last call."""
        a, b = C.c_float(), C.c_float()
        if lib().mwx_vad_last_kernel_ms(self.vctx, C.byref(a), C.byref(b)) != 0:
            raise RuntimeError("mwx_vad_last_kernel_ms: no timed call")
        return a.value, b.value

    # ---- speech segments and trimming ----
    @staticmethod
    def _segments(handle) -> List[tuple]:
        """[(t0, t1), ...] in centiseconds (float) of an mwx_vad_segments; frees it."""
        L = lib()
        if not handle:
            raise RuntimeError("mwx_vad_segments_* failed")
        try:
            return [(L.mwx_vad_segments_get_segment_t0(handle, i),
                     L.mwx_vad_segments_get_segment_t1(handle, i))
                    for i in range(L.mwx_vad_segments_n_segments(handle))]
        finally:
            L.mwx_vad_free_segments(handle)

    def segments_from_probs(self, params: Optional[VadParams] = None) -> List[tuple]:
        """mwx_vad_segments_from_probs over the last detect()'s probabilities."""
        return self._segments(lib().mwx_vad_segments_from_probs(self.vctx, params or vad_params()))

    def segments_from_samples(self, pcm, params: Optional[VadParams] = None) -> List[tuple]:
        _keep, addr, n = self._clip(pcm)
        return self._segments(lib().mwx_vad_segments_from_samples(
            self.vctx, params or vad_params(), addr, n))

    def trim_batch(self, pcms, params: Optional[VadParams] = None,
                   chunk_s: Optional[float] = None) -> "VadTrimmed":
        """mwx_vad_trim_batch: VAD, segments and compaction of every clip. With
        chunk_s, mwx_vad_trim_batch_chunked: plus the chunk plan."""
        clips = [self._clip(p) for p in pcms]
        n = len(clips)
        ptrs = (C.c_void_p * max(n, 1))(*[c[1] for c in clips])
        lens = (C.c_int * max(n, 1))(*[c[2] for c in clips])
        if chunk_s is None:
            t = lib().mwx_vad_trim_batch(self.vctx, params or vad_params(), ptrs, lens, n)
        else:
            t = lib().mwx_vad_trim_batch_chunked(self.vctx, params or vad_params(), chunk_s, ptrs,
                                                 lens, n)
        if not t:
            raise RuntimeError("mwx_vad_trim_batch failed")
        return VadTrimmed(t)

    def last_chunk_kernel_ms(self) -> float:
        """vad_chunks_kernel's device milliseconds in the last chunked trim_batch."""
        a = C.c_float()
        if lib().mwx_vad_last_chunk_kernel_ms(self.vctx, C.byref(a)) != 0:
            raise RuntimeError("mwx_vad_last_chunk_kernel_ms: no timed call")
        return a.value

    def test_chunks(self, probs: Sequence[np.ndarray], n_samples: Sequence[int],
                    params: Sequence[VadParams], caps: Sequence[int]):
        """mwx_test_vad_chunks: vad_segments_kernel, then vad_chunks_kernel over
        given probabilities, clip b with cap caps[b] in samples. Per clip:
        [(first piece, n pieces, start, len), ...]."""
        n = len(probs)
        arrs = [np.ascontiguousarray(p, np.float32) for p in probs]
        offs = np.concatenate([[0], np.cumsum([len(a) for a in arrs])]).astype(np.int32)
        flat = np.concatenate(arrs + [np.zeros(1, np.float32)])
        ns = np.ascontiguousarray(n_samples, np.int32)
        cp = np.ascontiguousarray(caps, np.int64)
        prm = (VadParams * n)(*params)
        nch = np.zeros(n, np.int32)
        out = np.zeros(4 * max(1, int(offs[-1])), np.int64)
        ip, i64p = C.POINTER(C.c_int), C.POINTER(C.c_int64)
        rc = lib().mwx_test_vad_chunks(self.vctx, prm, cp.ctypes.data_as(i64p), fptr(flat),
                                       offs.ctypes.data_as(ip), ns.ctypes.data_as(ip), n,
                                       nch.ctypes.data_as(ip), out.ctypes.data_as(i64p),
                                       offs.ctypes.data_as(ip))
        if rc != 0:
            raise RuntimeError(f"mwx_test_vad_chunks failed ({rc})")
        return [[tuple(int(v) for v in out[4 * (int(offs[b]) + j):4 * (int(offs[b]) + j) + 4])
                 for j in range(int(nch[b]))] for b in range(n)]

    def last_trim_kernel_ms(self):
        """(segments, compaction) device milliseconds of the last trim_batch."""
        a, b = C.c_float(), C.c_float()
        if lib().mwx_vad_last_trim_kernel_ms(self.vctx, C.byref(a), C.byref(b)) != 0:
            raise RuntimeError("mwx_vad_last_trim_kernel_ms: no timed call")
        return a.value, b.value

    def stream(self, params: Optional[VadParams] = None) -> "VadStream":
        """mwx_vad_stream_init: a stream of this context."""
        return VadStream(self, params)

    def last_stream_kernel_ms(self):
        """(staging, front end, recurrence + head) device milliseconds of the
        last VadStream.feed_batch."""
        a, b, c = C.c_float(), C.c_float(), C.c_float()
        if lib().mwx_vad_stream_last_kernel_ms(self.vctx, C.byref(a), C.byref(b),
                                               C.byref(c)) != 0:
            raise RuntimeError("mwx_vad_stream_last_kernel_ms: no timed call")
        return a.value, b.value, c.value

    def test_stream_scan(self, probs: np.ndarray, splits: Sequence[int], params: VadParams):
        """mwx_test_vad_stream_scan: the online scan over given probabilities fed
        splits[k] chunks at a time. ([(s0, s1, closed_at)], (trig, start,
        temp_end, prev_end, next_start, chunk count))."""
        p = np.ascontiguousarray(probs, np.float32)
        flat = np.concatenate([p, np.zeros(1, np.float32)])
        sp = np.ascontiguousarray(splits, np.int32)
        n_ev = C.c_int()
        ev = np.zeros(3 * max(1, len(p)), np.int64)
        st = np.zeros(6, np.int64)
        ip, i64p = C.POINTER(C.c_int), C.POINTER(C.c_int64)
        rc = lib().mwx_test_vad_stream_scan(self.vctx, C.byref(params), fptr(flat), len(p),
                                            sp.ctypes.data_as(ip), len(sp), C.byref(n_ev),
                                            ev.ctypes.data_as(i64p), st.ctypes.data_as(i64p))
        if rc != 0:
            raise RuntimeError(f"mwx_test_vad_stream_scan failed ({rc})")
        return ([tuple(int(v) for v in ev[3 * k:3 * k + 3]) for k in range(n_ev.value)],
                tuple(int(v) for v in st))

    def test_segments(self, probs: Sequence[np.ndarray], n_samples: Sequence[int],
                      params: Sequence[VadParams]):
        """mwx_test_vad_segments: vad_segments_kernel over given probabilities.
        Per clip: (segments [(s, e)], pieces [(src, len, dst)], compacted length)."""
        n = len(probs)
        arrs = [np.ascontiguousarray(p, np.float32) for p in probs]
        counts = [len(a) for a in arrs]
        offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        flat = np.concatenate(arrs + [np.zeros(1, np.float32)])
        ns = np.ascontiguousarray(n_samples, np.int32)
        prm = (VadParams * n)(*params)
        nseg = np.zeros(n, np.int32)
        clen = np.zeros(n, np.int64)
        seg = np.zeros(2 * max(1, int(offs[-1])), np.int64)
        pcs = np.zeros(3 * max(1, int(offs[-1])), np.int64)
        ip, i64p = C.POINTER(C.c_int), C.POINTER(C.c_int64)
        rc = lib().mwx_test_vad_segments(self.vctx, prm, fptr(flat), offs.ctypes.data_as(ip),
                                         ns.ctypes.data_as(ip), n, nseg.ctypes.data_as(ip),
                                         clen.ctypes.data_as(i64p), seg.ctypes.data_as(i64p),
                                         pcs.ctypes.data_as(i64p), offs.ctypes.data_as(ip))
        if rc != 0:
            raise RuntimeError(f"mwx_test_vad_segments failed ({rc})")
        out = []
        for b in range(n):
            o, m = int(offs[b]), int(nseg[b])
            out.append(([tuple(int(v) for v in seg[2 * (o + k):2 * (o + k) + 2]) for k in range(m)],
                        [tuple(int(v) for v in pcs[3 * (o + k):3 * (o + k) + 3]) for k in range(m)],
                        int(clen[b])))
        return out


class VadStream:
    """mwx_vad_stream: a VAD that is fed a piece at a time. Its
    probabilities are, bit for bit, VadContext.detect of everything fed since
    the last reset; its segments are rule D7's raw (unpadded) segments. Belongs
    to its VadContext (one call at a time per context); free it first."""

    def __init__(self, vad: "VadContext", params: Optional[VadParams] = None):
        self.vad = vad
        self.s = lib().mwx_vad_stream_init(vad.vctx, params or vad_params())
        if not self.s:
            raise RuntimeError("mwx_vad_stream_init failed")

    def free(self):
        if self.s:
            lib().mwx_vad_stream_free(self.s)
            self.s = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()

    def reset(self) -> None:
        if lib().mwx_vad_stream_reset(self.s) != 0:
            raise RuntimeError("mwx_vad_stream_reset failed")

    def feed(self, pcm) -> None:
        """mwx_vad_stream_feed_batch with this stream alone."""
        VadStream.feed_batch([self], [pcm])

    @staticmethod
    def feed_batch(streams: Sequence["VadStream"], pcms) -> None:
        """mwx_vad_stream_feed_batch: pcms[i] (numpy or DevicePCM, may be empty)
        is appended to streams[i], all in one pass. Streams of one context."""
        n = len(streams)
        if n == 0:
            return
        clips = [VadContext._clip(p) for p in pcms]
        hs = (C.c_void_p * n)(*[s.s for s in streams])
        ptrs = (C.c_void_p * n)(*[c[1] for c in clips])
        lens = (C.c_int * n)(*[c[2] for c in clips])
        rc = lib().mwx_vad_stream_feed_batch(streams[0].vad.vctx, hs, ptrs, lens, n)
        if rc != 0:
            raise RuntimeError(f"mwx_vad_stream_feed_batch failed ({rc})")

    def finish(self) -> None:
        if lib().mwx_vad_stream_finish(self.s) != 0:
            raise RuntimeError("mwx_vad_stream_finish failed")

    @property
    def n_samples(self) -> int:
        return lib().mwx_vad_stream_n_samples(self.s)

    @property
    def n_probs(self) -> int:
        return lib().mwx_vad_stream_n_probs(self.s)

    def probs(self) -> np.ndarray:
        k = self.n_probs
        if k == 0:
            return np.empty(0, np.float32)
        return np.ctypeslib.as_array(lib().mwx_vad_stream_probs(self.s), shape=(k,)).copy()

    @property
    def max_prob(self) -> float:
        return lib().mwx_vad_stream_max_prob(self.s)

    @property
    def in_speech(self) -> bool:
        return bool(lib().mwx_vad_stream_in_speech(self.s))

    def segments(self) -> List[tuple]:
        """[(s0, s1, closed_at), ...]: the raw segments closed since reset."""
        L = lib()
        out = []
        for i in range(L.mwx_vad_stream_n_segments(self.s)):
            a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
            if L.mwx_vad_stream_segment(self.s, i, C.byref(a), C.byref(b), C.byref(c)) != 0:
                raise RuntimeError("mwx_vad_stream_segment failed")
            out.append((a.value, b.value, c.value))
        return out


def vad_params(**kw) -> VadParams:
    """mwx_vad_default_params with fields replaced."""
    p = lib().mwx_vad_default_params()
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


class VadTrimmed:
    """mwx_vad_trimmed: the speech segments of every clip of a trim_batch call
    and the compacted PCM on the device. Independent of its VadContext."""

    def __init__(self, handle):
        self.t = handle

    def free(self):
        if self.t:
            lib().mwx_vad_trimmed_free(self.t)
            self.t = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()

    def __len__(self):
        return lib().mwx_vad_trimmed_n_clips(self.t)

    def segments(self, clip: int) -> List[tuple]:
        """[(start, end), ...] in samples of the caller's clip."""
        L = lib()
        out = []
        for i in range(L.mwx_vad_trimmed_n_segments(self.t, clip)):
            a, b = C.c_int64(), C.c_int64()
            if L.mwx_vad_trimmed_segment(self.t, clip, i, C.byref(a), C.byref(b)) != 0:
                raise RuntimeError("mwx_vad_trimmed_segment failed")
            out.append((a.value, b.value))
        return out

    def n_samples(self, clip: int) -> int:
        return lib().mwx_vad_trimmed_n_samples(self.t, clip)

    def map_time(self, clip: int, t_cs: int, is_end: bool) -> int:
        return lib().mwx_vad_trimmed_map_time(self.t, clip, t_cs, is_end)

    def chunks(self, clip: int) -> List[tuple]:
        """[(first segment, n segments, start, len), ...]: the clip's chunk plan,
        start and len in samples of the compacted clip."""
        L = lib()
        out = []
        for j in range(L.mwx_vad_trimmed_n_chunks(self.t, clip)):
            f, n, a, b = C.c_int(), C.c_int(), C.c_int64(), C.c_int64()
            if L.mwx_vad_trimmed_chunk(self.t, clip, j, C.byref(f), C.byref(n), C.byref(a),
                                       C.byref(b)) != 0:
                raise RuntimeError("mwx_vad_trimmed_chunk failed")
            out.append((f.value, n.value, a.value, b.value))
        return out

    def chunk_map_time(self, clip: int, j: int, t_cs: int, is_end: bool) -> int:
        return lib().mwx_vad_trimmed_chunk_map_time(self.t, clip, j, t_cs, is_end)

    def pcm(self, clip: int) -> np.ndarray:
        """mwx_test_vad_trimmed_pcm: the compacted clip, copied to the host."""
        n = self.n_samples(clip)
        out = np.empty(max(n, 1), np.float32)
        r = lib().mwx_test_vad_trimmed_pcm(self.t, clip, fptr(out), n)
        if r != n:
            raise RuntimeError(f"mwx_test_vad_trimmed_pcm returned {r}")
        return out[:n].copy()


def read_hparams(path: str) -> List[int]:
    with open(path, "rb") as f:
        b = f.read(48)
    return list(np.frombuffer(b[4:48], dtype=np.int32))


def token_ids(segs: List[Segment]) -> List[int]:
    return [t.id for s in segs for t in s.tokens]
