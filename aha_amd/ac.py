"""Host-side mirror of the reference's public API for the accelerated path:
``Aha::AC.compile`` / ``#match`` / ``Aha::Hit`` (src/aha/ac.cr:62-112, 280-295,
321-364; src/aha/matcher.cr:2-46), backed by libaha_hip.so through the C ABI.

Names, argument meaning and error behaviour follow the reference so that the
parity tests read like spec/ac_spec.cr:

    matcher = AC.compile(["我", "我是", "是中"])
    for hit in matcher.match("我是中国人"):
        hit.end, hit.value

``str`` input is the ``String`` overload (char offsets), ``bytes`` the
``Bytes`` overload (byte offsets), a list of 1-char strings the ``Array(Char)``
overload.  There is no CPU fallback: matching needs a HIP device.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _native as N

#: Aha::Hit -- src/aha/matcher.cr:2-11
Hit = namedtuple("Hit", ["start", "end", "value"])

HIT_DTYPE = np.dtype([("start", "<i4"), ("end", "<i4"), ("value", "<i4")])
KEY_COUNT_DTYPE = np.dtype([("key", "<i4"), ("count", "<u4")])  # aha_key_count (document counts)


class AhaError(RuntimeError):
    """The reference raises plain Strings; ``code`` is the C-ABI status."""

    def __init__(self, code, message=None, key_index=None):
        self.code = code
        self.key_index = key_index
        super().__init__(message or N.lib().aha_strerror(code).decode())


class BitArray:
    """Minimal stand-in for Crystal's BitArray as used by match(seq, sep)."""

    def __init__(self, size):
        self.size = int(size)
        self._bits = bytearray((max(self.size, 1) + 7) // 8)

    def __setitem__(self, i, v):
        if not 0 <= i < self.size:
            raise IndexError(i)
        if v:
            self._bits[i >> 3] |= 1 << (i & 7)
        else:
            self._bits[i >> 3] &= ~(1 << (i & 7))

    def __getitem__(self, i):
        if not 0 <= i < self.size:
            raise IndexError(i)
        return bool((self._bits[i >> 3] >> (i & 7)) & 1)


def _b(x):
    if isinstance(x, str):
        return x.encode("utf-8")
    return bytes(x)


def _pack_keys(keys):
    ks = [_b(k) for k in keys]
    offs = np.zeros(len(ks) + 1, dtype=np.uint64)
    if ks:
        offs[1:] = np.cumsum([len(k) for k in ks], dtype=np.uint64)
    blob = np.frombuffer(b"".join(ks), dtype=np.uint8) if ks else np.zeros(0, np.uint8)
    return blob, offs


def _fill_byte(fill):
    """a fill given as an int, one byte or a one-byte str -> 0 .. 255"""
    if isinstance(fill, str):
        fill = fill.encode("utf-8")
    if isinstance(fill, (bytes, bytearray)):
        if len(fill) != 1:
            raise ValueError("fill must be one byte")
        return fill[0]
    return int(fill) & 0xFF


def _delim_byte(delim):
    """a record delimiter -- one byte as bytes, a one-byte str or an int -- as an int"""
    if isinstance(delim, str):
        delim = delim.encode("utf-8")
    if isinstance(delim, (bytes, bytearray)):
        if len(delim) != 1:
            raise ValueError("the record delimiter is one byte")
        return delim[0]
    if not 0 <= int(delim) <= 255:
        raise ValueError("the record delimiter is one byte")
    return int(delim)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


def _dptr(t):
    """a torch tensor's device address, or None"""
    return t.data_ptr() if t is not None else None


def _params(chars, sep, longest=0):
    p = N.aha_match_params()
    p.struct_size = C.sizeof(N.aha_match_params)
    p.char_offsets = 1 if chars else 0
    p.longest = int(longest)
    p.sep_size = 0
    if sep is not None:
        p.sep_size = sep.size
        n = min(len(sep._bits), 32)
        for i in range(n):
            p.sep_bits[i] = sep._bits[i]
    return p


def char_offsets_of(text, hits):
    """The byte offsets of a HIT_DTYPE array over the UTF-8 bytes `text` as character offsets: the character index of a
    byte offset is the number of lead bytes (anything but 0b10xxxxxx) in front of it -- a running count."""
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    lead = np.zeros(t.size + 1, dtype=np.int64)
    np.cumsum((t & 0xC0) != 0x80, out=lead[1:])
    out = np.array(hits, dtype=HIT_DTYPE)
    out["start"] = lead[np.asarray(hits["start"], dtype=np.int64)]
    out["end"] = lead[np.asarray(hits["end"], dtype=np.int64)]
    return out


def _replacement_of(repl, key, n_keys):
    if hasattr(repl, "keys"):
        return repl.get(key)  # a mapping: keys it does not name stay as they are
    if len(repl) != n_keys:
        raise ValueError("repl must have one entry per key (%d), or be a mapping from key index" % n_keys)
    return repl[key]


def substitute(text, hits, repl, n_keys):
    """`text` (bytes) with every hit of `hits` (ascending, non-overlapping byte offsets: a selection) replaced by
    repl[hit.value]; repl: a mapping from key index to replacement (a key it does not name, or that maps to None, is left
    as it is) or a sequence with one entry per key.  Replacements are bytes or str (UTF-8).  -> bytes"""
    text = bytes(text)
    parts, at = [], 0
    for s, e, v in np.asarray(hits).tolist():
        r = _replacement_of(repl, v, n_keys)
        if r is None:
            continue
        parts.append(text[at:s])
        parts.append(_b(r))
        at = e
    parts.append(text[at:])
    return b"".join(parts)


class ReplTable:
    """A replacement table of one handle (aha_repl_create): validated and uploaded once, immutable, freed with the object.
    Made by AC.replacements."""

    def __init__(self, handle, n_keys):
        self._h, self.n_keys = handle, n_keys

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                N.lib().aha_repl_free(h)
            except Exception:  # interpreter shutdown
                pass


class Classes:
    """A class table of one handle (aha_classes_create): per key its classes, validated and uploaded once, immutable, freed
    with the object.  Made by AC.classes.  n_classes = C; names: the class names in column order where the spec gave
    names, else None."""

    def __init__(self, handle, n_keys, n_classes, names=None):
        self._h, self.n_keys, self.n_classes, self.names = handle, n_keys, n_classes, names

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                N.lib().aha_classes_free(h)
            except Exception:  # interpreter shutdown
                pass


class Rule:
    """A rule over class counts for the grep calls (AHA_GREP_RULE), validated on the host and immutable.  Made by AC.rule.
    classes: the Classes it names; terms: a tuple of (class_id, op, group, num, den_bytes) with op 0 for >= and 1 for <; a
    document passes when some group has all its terms true."""

    __slots__ = ("classes", "terms", "_arr")

    def __init__(self, classes, terms):
        object.__setattr__(self, "classes", classes)
        object.__setattr__(self, "terms", tuple(terms))
        arr = (N.aha_rule_term * len(self.terms))()
        for i, (c, op, g, num, den) in enumerate(self.terms):
            arr[i] = N.aha_rule_term(c, op, g, num, den)
        object.__setattr__(self, "_arr", arr)

    def __setattr__(self, name, value):
        raise AttributeError("a Rule is immutable")

    def __repr__(self):
        return "Rule(%r)" % (self.terms,)


def _pack_replacements(repl, n_keys):
    """repl as substitute takes it -> (blob uint8, offsets uint64[K+1], keep bits uint32[ceil(K/32)])"""
    parts, keep = [], np.zeros((n_keys + 31) // 32, dtype=np.uint32)
    offs = np.zeros(n_keys + 1, dtype=np.uint64)
    if hasattr(repl, "keys"):
        for k in repl.keys():
            if not 0 <= int(k) < n_keys:
                raise ValueError("repl names key %r; the handle has %d keys" % (k, n_keys))
    at = 0
    for k in range(n_keys):
        r = _replacement_of(repl, k, n_keys)
        if r is None:
            keep[k >> 5] |= np.uint32(1 << (k & 31))
        else:
            r = _b(r)
            parts.append(r)
            at += len(r)
        offs[k + 1] = at
    blob = np.frombuffer(b"".join(parts), dtype=np.uint8) if at else np.zeros(0, np.uint8)
    return blob, offs, keep


class AC:
    """Aha::AC (= ACX(Int32), src/aha/ac.cr:8-11) on the MI355X."""

    def __init__(self, handle):
        self._h = handle

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                N.lib().aha_ac_free(h)
            except Exception:  # interpreter shutdown: the module globals may already be gone
                pass

    # -- Aha::AC.compile(keys) src/aha/ac.cr:62-69 ---------------------------
    @classmethod
    def compile(cls, keys, device=-1, host_only=False, force_wide=False, fold_ascii=False, fold_simple=False, fold_bmp=False,
                fold_kana=False):
        """fold_kana: fold_bmp plus hiragana and half-width katakana matched as katakana (AHA_OPT_FOLD_KANA: length-preserving, so
        a half-width letter and its voiced mark stay two characters; small and large kana stay apart; the same limits).
        fold_bmp: fold_simple plus the three-byte UTF-8 characters (AHA_OPT_FOLD_BMP: full-width Latin, Vietnamese, polytonic
        Greek, Georgian, Cherokee, Glagolitic, Coptic ..; the same limits).
        fold_simple: fold_ascii plus the simple case fold of the two-byte UTF-8 characters (AHA_OPT_FOLD_SIMPLE: Latin-1,
        Latin Extended-A/B, Greek, Cyrillic, Armenian; every document folded on its own; no feeds and no groups yet).
        fold_ascii: an ASCII case-insensitive handle (AHA_OPT_FOLD_ASCII, include/aha_hip.h): every call gives what a plain
        handle compiled from the lower-cased keys gives over the lower-cased text ('A'..'Z' only; offsets are the original
        text's); `redact` keeps the original bytes outside the hits, `m[id]` the keys as spelled here."""
        blob, offs = _pack_keys(keys)
        return cls.compile_packed(blob, offs, device, host_only, force_wide, fold_ascii, fold_simple, fold_bmp, fold_kana)

    @classmethod
    def compile_packed(cls, blob, offs, device=-1, host_only=False, force_wide=False, fold_ascii=False, fold_simple=False,
                       fold_bmp=False, fold_kana=False):
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        opts = N.aha_options()
        opts.struct_size = C.sizeof(N.aha_options)
        opts.device = device
        opts.flags = ((N.AHA_OPT_HOST_ONLY if host_only else 0) | (N.AHA_OPT_FORCE_WIDE if force_wide else 0) |
                      (N.AHA_OPT_FOLD_ASCII if fold_ascii else 0) | (N.AHA_OPT_FOLD_SIMPLE if fold_simple else 0) |
                      (N.AHA_OPT_FOLD_BMP if fold_bmp else 0) | (N.AHA_OPT_FOLD_KANA if fold_kana else 0))
        h = C.c_void_p()
        ek = C.c_uint32(0)
        rc = N.lib().aha_ac_compile(_ptr(blob), _ptr(offs), len(offs) - 1, C.byref(opts), C.byref(h),
                                    C.byref(ek))
        if rc != N.AHA_OK:
            msg = None
            if rc == N.AHA_E_DUP_KEY:  # raise "key:#{key} appear twice." ac.cr:66
                k = bytes(blob[int(offs[ek.value]):int(offs[ek.value + 1])])
                msg = f"key:{k.decode('utf-8', 'replace')} appear twice."
            raise AhaError(rc, msg, ek.value)
        return cls(h)

    # -- AC#save(io) / AC.load(io): src/aha/ac.cr:45-60 (own container, see include/aha_hip.h) --
    def to_bytes(self):
        n = N.lib().aha_ac_save(self._h, None, 0)
        if n < 0:
            raise AhaError(int(n))
        buf = np.zeros(int(n), dtype=np.uint8)
        got = N.lib().aha_ac_save(self._h, _ptr(buf), int(n))
        assert got == n
        return buf.tobytes()

    def save(self, io):
        """io: a path or a binary file object."""
        data = self.to_bytes()
        if hasattr(io, "write"):
            io.write(data)
        else:
            with open(io, "wb") as f:
                f.write(data)

    @classmethod
    def from_bytes(cls, data, device=-1, host_only=False, force_wide=False, fold_ascii=False, fold_simple=False, fold_bmp=False,
                   fold_kana=False):
        """The container stores the keys as they were spelled and no options: say fold_ascii / fold_simple / fold_bmp / fold_kana again, like
        force_wide."""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        opts = N.aha_options()
        opts.struct_size = C.sizeof(N.aha_options)
        opts.device = device
        opts.flags = ((N.AHA_OPT_HOST_ONLY if host_only else 0) | (N.AHA_OPT_FORCE_WIDE if force_wide else 0) |
                      (N.AHA_OPT_FOLD_ASCII if fold_ascii else 0) | (N.AHA_OPT_FOLD_SIMPLE if fold_simple else 0) |
                      (N.AHA_OPT_FOLD_BMP if fold_bmp else 0) | (N.AHA_OPT_FOLD_KANA if fold_kana else 0))
        h = C.c_void_p()
        rc = N.lib().aha_ac_load(_ptr(buf), buf.size, C.byref(opts), C.byref(h))
        if rc != N.AHA_OK:
            raise AhaError(rc, "not an aha_hip automaton file" if rc == N.AHA_E_INVALID else None)
        return cls(h)

    @classmethod
    def load(cls, io, **kw):
        if hasattr(io, "read"):
            return cls.from_bytes(io.read(), **kw)
        with open(io, "rb") as f:
            return cls.from_bytes(f.read(), **kw)

    def _check(self, rc):
        if rc != N.AHA_OK:
            msg = N.lib().aha_last_error(self._h).decode() or None
            raise AhaError(rc, msg)

    @property
    def info(self):
        i = N.aha_ac_info_t()
        i.struct_size = C.sizeof(i)  # (in: the bytes this binding's struct has; the library fills no more)
        self._check(N.lib().aha_ac_info(self._h, C.byref(i)))
        return {f: getattr(i, f) for f, _ in i._fields_ if f != "struct_size"}

    @property
    def fold_ascii(self):
        """True for a handle compiled (or loaded) with fold_ascii=True."""
        return bool(N.lib().aha_ac_flags(self._h) & N.AHA_OPT_FOLD_ASCII)

    @property
    def fold_simple(self):
        """True for a handle compiled (or loaded) with fold_simple=True."""
        return bool(N.lib().aha_ac_flags(self._h) & N.AHA_OPT_FOLD_SIMPLE)

    @property
    def fold_bmp(self):
        """True for a handle compiled (or loaded) with fold_bmp=True."""
        return bool(N.lib().aha_ac_flags(self._h) & N.AHA_OPT_FOLD_BMP)

    @property
    def fold_kana(self):
        """True for a handle compiled (or loaded) with fold_kana=True."""
        return bool(N.lib().aha_ac_flags(self._h) & N.AHA_OPT_FOLD_KANA)

    # -- delegate :[] src/aha/ac.cr:41-43 ------------------------------------
    def __getitem__(self, x):
        if isinstance(x, (int, np.integer)):
            buf = C.create_string_buffer(1 << 12)
            n = N.lib().aha_ac_key(self._h, int(x), buf, len(buf))
            if n > len(buf):
                buf = C.create_string_buffer(n)
                n = N.lib().aha_ac_key(self._h, int(x), buf, len(buf))
            if n < 0:
                raise IndexError(x)
            return buf.raw[:n].decode("utf-8", "replace")
        k = _b(x)
        r = N.lib().aha_ac_id(self._h, k, len(k))
        if r < 0:
            raise IndexError(x)  # IndexError.new cedar.cr:832
        return r

    # -- #match ---------------------------------------------------------------
    def match_array(self, seq, sep=None, chars=None, longest=0):
        """All hits of one sequence as a HIT_DTYPE array (reference order)."""
        if isinstance(seq, (list, tuple)) and (not seq or isinstance(seq[0], str)):
            if sep is not None:
                return self._match_chars_sep(list(seq), sep)
            # Array(Char) overload (ac.cr:288-295): chars re-encode to UTF-8
            seq = "".join(seq)
        if chars is None:
            chars = isinstance(seq, str)
        t = np.frombuffer(_b(seq), dtype=np.uint8)
        p = _params(chars, sep, longest)
        cap = max(64, t.size // 4)
        while True:
            out = np.zeros(cap, dtype=HIT_DTYPE)
            n = C.c_uint64(0)
            rc = N.lib().aha_ac_match_bytes(self._h, _ptr(t), t.size, C.byref(p), _ptr(out), cap, C.byref(n))
            if rc == N.AHA_E_CAPACITY:
                cap = int(n.value)
                continue
            self._check(rc)
            return out[: n.value]

    def _match_chars_sep(self, chars, sep):
        """match(seq : Array(Char) | Slice(Char), sep) -- src/aha/ac.cr:342-364.  Unlike the String overload
        (matcher.cr:41-46, byte-level neighbours) this one tests the neighbouring CODE POINT: a hit is dropped when
        `chr.ord < sep.size && !sep[chr.ord]`, so a neighbour whose code point is >= sep.size never blocks.  The GPU
        yields the unfiltered byte-offset hits; the two neighbour tests and the char offsets are applied here."""
        if sep.size > 256:
            raise AhaError(N.AHA_E_SEP_SIZE, "sep BitArray size > 256 is not supported")
        enc = [c.encode("utf-8") for c in chars]
        t = b"".join(enc)
        hits = self.match_array(t, None, False)
        if not len(hits):
            return hits
        cps = np.array([ord(c) for c in chars], dtype=np.int64)
        blens = np.array([len(e) for e in enc], dtype=np.int64)
        char_of_byte = np.repeat(np.arange(len(chars), dtype=np.int64), blens)
        ok_cp = np.array([not (i < sep.size and not sep[i]) for i in range(256)], dtype=bool)  # blocked(c) for c < 256
        blocked = (cps < 256) & ~ok_cp[np.minimum(cps, 255)]
        nchars = len(chars)
        end_chr = char_of_byte[hits["end"].astype(np.int64) - 1]      # char that holds the last byte (ac.cr:346)
        right = end_chr + 1
        keep = ~((right < nchars) & blocked[np.minimum(right, nchars - 1)])
        start_chr = char_of_byte[hits["start"].astype(np.int64)]
        has_left = hits["start"] > 0                                    # ac.cr:354
        keep &= ~(has_left & blocked[np.maximum(start_chr - 1, 0)])
        out = np.zeros(int(keep.sum()), dtype=HIT_DTYPE)
        out["start"] = start_chr[keep]
        out["end"] = end_chr[keep] + 1
        out["value"] = hits["value"][keep]
        return out

    def match(self, seq, sep=None, chars=None):
        """Yields Aha::Hit like the reference's block form (ac.cr:280-286)."""
        for s, e, v in self.match_array(seq, sep, chars).tolist():
            yield Hit(s, e, v)

    def match_longest(self, seq, intersectable=False, chars=None):
        """ACX#match_longest(seq, intersectable = false) -- src/aha/ac.cr:297-319."""
        for s, e, v in self.match_array(seq, None, chars, longest=2 if intersectable else 1).tolist():
            yield Hit(s, e, v)

    def match_batch(self, corpus, doc_offsets, sep=None, chars=False, cap=None, longest=0):
        """D documents in one call: returns (hits, doc_hit_offsets).  longest: 0 = #match, 1 / 2 = #match_longest
        with intersectable false / true."""
        if isinstance(corpus, (bytes, bytearray)):
            corpus = np.frombuffer(bytes(corpus), dtype=np.uint8)
        corpus = np.ascontiguousarray(corpus, dtype=np.uint8)
        doc_offsets = np.ascontiguousarray(doc_offsets, dtype=np.uint64)
        D = doc_offsets.size - 1
        p = _params(chars, sep, longest)
        dho = np.zeros(D + 1, dtype=np.uint64)
        if cap is None:
            cap = max(64, corpus.size // 8)
        while True:
            out = np.zeros(cap, dtype=HIT_DTYPE)
            n = C.c_uint64(0)
            rc = N.lib().aha_ac_match_batch(self._h, _ptr(corpus), _ptr(doc_offsets), D, C.byref(p), _ptr(out),
                                            cap, _ptr(dho), C.byref(n))
            if rc == N.AHA_E_CAPACITY:
                cap = int(n.value)
                continue
            self._check(rc)
            return out[: n.value], dho

    def match_batch_device(self, corpus, doc_offsets, out, doc_hit_offsets=None, sep=None, chars=False,
                           stream=None, words=None, n_words=None, longest=0):
        """Device-resident batch match on torch CUDA tensors (uint8 corpus,
        int64/uint64 doc offsets, int32 [cap,3] out).  Returns the hit count;
        raises AhaError(AHA_E_CAPACITY) with .required when out is too small.
        longest: as in match_batch.
        words (int32, >= 2 cap + cap / 1024 + 2 elements) + n_words (int64[1]): the hits also as the 4-byte exchange stream
        (aha_ac_match_batch_device_stream: written by the expansion itself where the character-level engine runs)."""
        import torch

        assert corpus.is_cuda and corpus.dtype == torch.uint8 and corpus.is_contiguous()
        assert doc_offsets.is_cuda and doc_offsets.dtype in (torch.int64, torch.uint64)
        assert out.is_cuda and out.dtype == torch.int32 and out.is_contiguous()
        D = doc_offsets.numel() - 1
        cap = out.numel() // 3
        p = _params(chars, sep, longest)
        n = C.c_uint64(0)
        s = stream if stream is not None else torch.cuda.current_stream(corpus.device).cuda_stream
        dho = doc_hit_offsets.data_ptr() if doc_hit_offsets is not None else None
        if words is not None:
            assert words.is_cuda and words.dtype == torch.int32 and n_words.is_cuda and n_words.dtype == torch.int64
            rc = N.lib().aha_ac_match_batch_device_stream(self._h, corpus.data_ptr(), doc_offsets.data_ptr(), D, corpus.numel(),
                                                          C.byref(p), out.data_ptr(), cap, dho, C.byref(n), words.data_ptr(),
                                                          words.numel(), n_words.data_ptr(), C.c_void_p(s))
        else:
            rc = N.lib().aha_ac_match_batch_device(self._h, corpus.data_ptr(), doc_offsets.data_ptr(), D,
                                                   corpus.numel(), C.byref(p), out.data_ptr(), cap, dho,
                                                   C.byref(n), C.c_void_p(s))
        if rc == N.AHA_E_CAPACITY:
            e = AhaError(rc)
            e.required = int(n.value)
            raise e
        self._check(rc)
        return int(n.value)

    def match_batch_keep(self, corpus, doc_offsets, d_hits, chars=False):
        """aha_ac_match_batch_keep: host corpus in (uploaded range by range beside the matches), the hits stay on the device in
        d_hits (a torch int32 [cap, 3] tensor on the handle's device); returns (n_hits, per-document offsets)."""
        corpus = np.ascontiguousarray(corpus, dtype=np.uint8)
        doc_offsets = np.ascontiguousarray(doc_offsets, dtype=np.uint64)
        D = doc_offsets.size - 1
        p = _params(chars, None)
        dho = np.zeros(D + 1, dtype=np.uint64)
        n = C.c_uint64(0)
        rc = N.lib().aha_ac_match_batch_keep(self._h, _ptr(corpus), _ptr(doc_offsets), D, C.byref(p),
                                             C.c_void_p(d_hits.data_ptr()), d_hits.shape[0], _ptr(dho), C.byref(n))
        if rc == N.AHA_E_CAPACITY:
            e = AhaError(rc)
            e.required = int(n.value)
            raise e
        self._check(rc)
        return int(n.value), dho

    def replicate(self, device):
        """aha_ac_replicate: a second handle for the same keys on another device -- the host image is copied and uploaded,
        nothing is compiled again."""
        h = C.c_void_p()
        rc = N.lib().aha_ac_replicate(self._h, device, C.byref(h))
        if rc != N.AHA_OK:
            raise AhaError(rc)
        return AC(h)

    def match_corpus(self, corpus, cap=None, sep=None, chars=False, longest=0):
        """Matches a batch that already lives in HBM (DeviceCorpus: uploaded once through the C ABI, no GPU framework
        involved) and downloads the hits: -> (hits, doc_hit_offsets).  The upload is not repeated per call."""
        D = corpus.n_docs
        if cap is None:
            cap = max(64, corpus.n_bytes // 8)
        p = _params(chars, sep, longest)
        dev = corpus.device
        dho = DeviceBuffer(dev, (D + 1) * 8)
        while True:
            out = DeviceBuffer(dev, cap * 12)
            n = C.c_uint64(0)
            rc = N.lib().aha_ac_match_batch_device(self._h, corpus.ptr, corpus.doc_ptr, D, corpus.n_bytes, C.byref(p),
                                                   out.ptr, cap, dho.ptr, C.byref(n), None)
            if rc == N.AHA_E_CAPACITY:
                cap = int(n.value)
                continue
            self._check(rc)
            return out.download(np.zeros(int(n.value), dtype=HIT_DTYPE)), dho.download(np.zeros(D + 1, dtype=np.uint64))

    # -- counts without the hit list (aha_ac_count_batch*) -------------------------------------------
    def count_batch(self, corpus, doc_offsets, sep=None, chars=False, per_key=True, accumulate_into=None):
        """Hits per key and per document of match_batch(corpus, doc_offsets, sep) without the hit list:
        -> (key_counts uint64[K] or None, doc_hit_offsets uint64[D+1]).  chars changes no count (accepted for symmetry).
        accumulate_into: a uint64[K] array the counts are added to (AHA_COUNT_ACCUMULATE); it is also what is returned."""
        if isinstance(corpus, (bytes, bytearray)):
            corpus = np.frombuffer(bytes(corpus), dtype=np.uint8)
        corpus = np.ascontiguousarray(corpus, dtype=np.uint8)
        doc_offsets = np.ascontiguousarray(doc_offsets, dtype=np.uint64)
        D = doc_offsets.size - 1
        p = _params(chars, sep)
        dho = np.zeros(D + 1, dtype=np.uint64)
        flags = 0
        kc = None
        if accumulate_into is not None:
            kc = accumulate_into
            if not (isinstance(kc, np.ndarray) and kc.dtype == np.uint64 and kc.flags.c_contiguous and kc.flags.writeable
                    and kc.size == self.n_keys):
                raise ValueError(f"accumulate_into must be a writeable C-contiguous uint64 array of {self.n_keys} entries")
            flags = N.AHA_COUNT_ACCUMULATE
        elif per_key:
            kc = np.zeros(self.n_keys, dtype=np.uint64)
        n = C.c_uint64(0)
        rc = N.lib().aha_ac_count_batch(self._h, _ptr(corpus), _ptr(doc_offsets), D, C.byref(p), flags, _ptr(kc), _ptr(dho),
                                        C.byref(n))
        self._check(rc)
        return kc, dho

    def count(self, seq, sep=None):
        """Hits per key of match(seq, sep) on one sequence: uint64[K]."""
        b = _b(seq)
        kc, _ = self.count_batch(np.frombuffer(b, dtype=np.uint8), np.array([0, len(b)], dtype=np.uint64), sep=sep)
        return kc

    def count_batch_device(self, corpus, doc_offsets, key_counts=None, doc_hit_offsets=None, sep=None, chars=False,
                           accumulate=False, stream=None):
        """Device-resident count on torch CUDA tensors (uint8 corpus, int64/uint64 doc offsets; key_counts int64/uint64 [K] or
        None; doc_hit_offsets int64/uint64 [D+1] or None).  Returns the hit count.  accumulate: add into key_counts."""
        import torch

        assert corpus.is_cuda and corpus.dtype == torch.uint8 and corpus.is_contiguous()
        assert doc_offsets.is_cuda and doc_offsets.dtype in (torch.int64, torch.uint64)
        if key_counts is not None and not (key_counts.is_cuda and key_counts.dtype in (torch.int64, torch.uint64)
                                           and key_counts.is_contiguous() and key_counts.numel() >= self.n_keys):
            raise ValueError(f"key_counts must be a contiguous int64/uint64 CUDA tensor of at least {self.n_keys} entries")
        if doc_hit_offsets is not None and not (doc_hit_offsets.is_cuda and doc_hit_offsets.dtype in (torch.int64, torch.uint64)
                                                and doc_hit_offsets.is_contiguous()
                                                and doc_hit_offsets.numel() >= doc_offsets.numel()):
            raise ValueError("doc_hit_offsets must be a contiguous int64/uint64 CUDA tensor of at least D + 1 entries")
        D = doc_offsets.numel() - 1
        p = _params(chars, sep)
        n = C.c_uint64(0)
        s = stream if stream is not None else torch.cuda.current_stream(corpus.device).cuda_stream
        kc = key_counts.data_ptr() if key_counts is not None else None
        dho = doc_hit_offsets.data_ptr() if doc_hit_offsets is not None else None
        rc = N.lib().aha_ac_count_batch_device(self._h, corpus.data_ptr(), doc_offsets.data_ptr(), D, corpus.numel(), C.byref(p),
                                               N.AHA_COUNT_ACCUMULATE if accumulate else 0, kc, dho, C.byref(n), C.c_void_p(s))
        self._check(rc)
        return int(n.value)

    def count_corpus(self, corpus, sep=None, chars=False, per_key=True):
        """Counts a batch that already lives in HBM (DeviceCorpus) and downloads the results:
        -> (key_counts uint64[K] or None, doc_hit_offsets uint64[D+1], n_hits)."""
        D = corpus.n_docs
        p = _params(chars, sep)
        dev = corpus.device
        dho = DeviceBuffer(dev, (D + 1) * 8)
        kc = DeviceBuffer(dev, max(1, self.n_keys) * 8) if per_key else None
        n = C.c_uint64(0)
        rc = N.lib().aha_ac_count_batch_device(self._h, corpus.ptr, corpus.doc_ptr, D, corpus.n_bytes, C.byref(p), 0,
                                               kc.ptr if kc else None, dho.ptr, C.byref(n), None)
        self._check(rc)
        counts = kc.download(np.zeros(self.n_keys, dtype=np.uint64)) if kc else None
        return counts, dho.download(np.zeros(D + 1, dtype=np.uint64)), int(n.value)

    # -- document counts: hits per key within each document (aha_ac_doc_counts_batch*) ---------------
    def doc_counts_batch(self, corpus, doc_offsets, sep=None, chars=False, cap=None):
        """The document x key table of match_batch(corpus, doc_offsets, sep) without the hit list:
        -> (pairs, doc_pair_offsets uint64[D+1]); pairs[doc_pair_offsets[d]:doc_pair_offsets[d+1]] holds document d's
        {key, count}, ascending by key.  cap None: a sizing call first.  chars changes no count."""
        if isinstance(corpus, (bytes, bytearray)):
            corpus = np.frombuffer(bytes(corpus), dtype=np.uint8)
        corpus = np.ascontiguousarray(corpus, dtype=np.uint8)
        doc_offsets = np.ascontiguousarray(doc_offsets, dtype=np.uint64)
        D = doc_offsets.size - 1
        p = _params(chars, sep)
        dpo = np.zeros(D + 1, dtype=np.uint64)
        n = C.c_uint64(0)
        L = N.lib()
        if cap is None:
            rc = L.aha_ac_doc_counts_batch(self._h, _ptr(corpus), _ptr(doc_offsets), D, C.byref(p), None, 0, _ptr(dpo),
                                           C.byref(n), None)
            if rc != N.AHA_E_CAPACITY:
                self._check(rc)
                return np.zeros(0, dtype=KEY_COUNT_DTYPE), dpo
            cap = int(n.value)
        out = np.zeros(max(int(cap), 1), dtype=KEY_COUNT_DTYPE)
        rc = L.aha_ac_doc_counts_batch(self._h, _ptr(corpus), _ptr(doc_offsets), D, C.byref(p), _ptr(out), int(cap), _ptr(dpo),
                                       C.byref(n), None)
        self._check(rc)
        return out[: int(n.value)], dpo

    def doc_counts(self, seq, sep=None):
        """Hits per key of match(seq, sep) on one sequence: {key id: count}."""
        b = _b(seq)
        pairs, _ = self.doc_counts_batch(np.frombuffer(b, dtype=np.uint8), np.array([0, len(b)], dtype=np.uint64), sep=sep)
        return {int(k): int(c) for k, c in zip(pairs["key"], pairs["count"])}

    def doc_counts_batch_device(self, corpus, doc_offsets, out, doc_pair_offsets=None, sep=None, chars=False, cap=None,
                                stream=None):
        """Device-resident document counts on torch CUDA tensors: uint8 corpus, int64/uint64 doc offsets, out int32 [cap, 2]
        ({key, count} rows) or None (a sizing call), doc_pair_offsets int64/uint64 [D+1] or None.
        -> (n_pairs, n_hits); raises AhaError(AHA_E_CAPACITY) when out is too small (e.n_required = the pairs needed)."""
        import torch

        assert corpus.is_cuda and corpus.dtype == torch.uint8 and corpus.is_contiguous()
        assert doc_offsets.is_cuda and doc_offsets.dtype in (torch.int64, torch.uint64)
        if out is not None:
            if not (out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and out.dim() == 2 and out.shape[1] == 2):
                raise ValueError("out must be a contiguous int32 CUDA tensor of shape [cap, 2]")
            cap = out.shape[0] if cap is None else min(int(cap), out.shape[0])
        else:
            cap = 0
        if doc_pair_offsets is not None and not (doc_pair_offsets.is_cuda and doc_pair_offsets.dtype in (torch.int64, torch.uint64)
                                                 and doc_pair_offsets.is_contiguous()
                                                 and doc_pair_offsets.numel() >= doc_offsets.numel()):
            raise ValueError("doc_pair_offsets must be a contiguous int64/uint64 CUDA tensor of at least D + 1 entries")
        D = doc_offsets.numel() - 1
        p = _params(chars, sep)
        n, nh = C.c_uint64(0), C.c_uint64(0)
        s = stream if stream is not None else torch.cuda.current_stream(corpus.device).cuda_stream
        rc = N.lib().aha_ac_doc_counts_batch_device(
            self._h, corpus.data_ptr(), doc_offsets.data_ptr(), D, corpus.numel(), C.byref(p),
            out.data_ptr() if out is not None and cap else None, cap,
            doc_pair_offsets.data_ptr() if doc_pair_offsets is not None else None, C.byref(n), C.byref(nh), C.c_void_p(s))
        if rc == N.AHA_E_CAPACITY:
            e = AhaError(rc, N.lib().aha_strerror(rc).decode())
            e.n_required = int(n.value)
            e.n_hits = int(nh.value)
            raise e
        self._check(rc)
        return int(n.value), int(nh.value)

    def doc_counts_corpus(self, corpus, sep=None, chars=False):
        """Document counts of a batch that already lives in HBM (DeviceCorpus), downloaded:
        -> (pairs, doc_pair_offsets uint64[D+1], n_hits)."""
        D = corpus.n_docs
        p = _params(chars, sep)
        dev = corpus.device
        dpo = DeviceBuffer(dev, (D + 1) * 8)
        n, nh = C.c_uint64(0), C.c_uint64(0)
        L = N.lib()
        rc = L.aha_ac_doc_counts_batch_device(self._h, corpus.ptr, corpus.doc_ptr, D, corpus.n_bytes, C.byref(p), None, 0,
                                              dpo.ptr, C.byref(n), C.byref(nh), None)
        if rc != N.AHA_E_CAPACITY:
            self._check(rc)
            return np.zeros(0, dtype=KEY_COUNT_DTYPE), dpo.download(np.zeros(D + 1, dtype=np.uint64)), int(nh.value)
        cap = int(n.value)
        out = DeviceBuffer(dev, cap * 8)
        rc = L.aha_ac_doc_counts_batch_device(self._h, corpus.ptr, corpus.doc_ptr, D, corpus.n_bytes, C.byref(p), out.ptr, cap,
                                              dpo.ptr, C.byref(n), C.byref(nh), None)
        self._check(rc)
        return (out.download(np.zeros(cap, dtype=KEY_COUNT_DTYPE)), dpo.download(np.zeros(D + 1, dtype=np.uint64)),
                int(nh.value))

    # -- select: leftmost-longest, non-overlapping hits per document (aha_ac_select_batch*) ----------
    def select_batch(self, corpus, doc_offsets, sep=None, cap=None, flags=0):
        """Per document the leftmost-longest, non-overlapping hits of match_batch(corpus, doc_offsets, sep), byte offsets:
        -> (hits HIT_DTYPE, doc_sel_offsets uint64[D+1]); hits[doc_sel_offsets[d]:doc_sel_offsets[d+1]] is document d's
        selection, ascending by start.  cap None: a sizing call first.  flags: AHA_SELECT_* (tokens_batch)."""
        if isinstance(corpus, (bytes, bytearray)):
            corpus = np.frombuffer(bytes(corpus), dtype=np.uint8)
        corpus = np.ascontiguousarray(corpus, dtype=np.uint8)
        doc_offsets = np.ascontiguousarray(doc_offsets, dtype=np.uint64)
        D = doc_offsets.size - 1
        p = _params(False, sep)
        dso = np.zeros(D + 1, dtype=np.uint64)
        n = C.c_uint64(0)
        L = N.lib()
        if cap is None:
            rc = L.aha_ac_select_batch(self._h, _ptr(corpus), _ptr(doc_offsets), D, C.byref(p), flags, None, 0, _ptr(dso),
                                       C.byref(n), None)
            if rc != N.AHA_E_CAPACITY:
                self._check(rc)
                return np.zeros(0, dtype=HIT_DTYPE), dso
            cap = int(n.value)
        out = np.zeros(max(int(cap), 1), dtype=HIT_DTYPE)
        rc = L.aha_ac_select_batch(self._h, _ptr(corpus), _ptr(doc_offsets), D, C.byref(p), flags, _ptr(out), int(cap), _ptr(dso),
                                   C.byref(n), None)
        if rc == N.AHA_E_CAPACITY:
            e = AhaError(rc, N.lib().aha_strerror(rc).decode())
            e.n_required = int(n.value)
            raise e
        self._check(rc)
        return out[: int(n.value)], dso

    def select_array(self, seq, sep=None):
        """The selection of one sequence as a HIT_DTYPE array: byte offsets for bytes, character offsets for str (the select
        runs over the UTF-8 bytes; the offsets are mapped here)."""
        b = _b(seq)
        hits, _ = self.select_batch(np.frombuffer(b, dtype=np.uint8), np.array([0, len(b)], dtype=np.uint64), sep=sep)
        return char_offsets_of(b, hits) if isinstance(seq, str) else hits

    def select(self, seq, sep=None):
        """The leftmost-longest, non-overlapping hits of match(seq, sep) as a list of Hit, ascending by start."""
        return [Hit(s, e, v) for s, e, v in self.select_array(seq, sep).tolist()]

    def replace(self, seq, repl, sep=None):
        """seq with every selected hit replaced by repl[hit.value]: repl is a mapping from key index to replacement (keys it
        does not name stay) or a sequence with one entry per key.  bytes in, bytes out; str in, str out.  The copy is built
        on the host from select."""
        b = _b(seq)
        hits, _ = self.select_batch(np.frombuffer(b, dtype=np.uint8), np.array([0, len(b)], dtype=np.uint64), sep=sep)
        out = substitute(b, hits, repl, self.n_keys)
        return out.decode("utf-8") if isinstance(seq, str) else out

    def select_batch_device(self, corpus, doc_offsets, out, doc_sel_offsets=None, sep=None, cap=None, stream=None, flags=0):
        """Device-resident select on torch CUDA tensors: uint8 corpus, int64/uint64 doc offsets, out int32 [cap, 3]
        ({start, end, value} rows) or None (a sizing call), doc_sel_offsets int64/uint64 [D+1] or None.
        -> (n_selected, n_hits); raises AhaError(AHA_E_CAPACITY) when out is too small (e.n_required = the hits needed);
        nothing is written then."""
        import torch

        assert corpus.is_cuda and corpus.dtype == torch.uint8 and corpus.is_contiguous()
        assert doc_offsets.is_cuda and doc_offsets.dtype in (torch.int64, torch.uint64)
        if out is not None:
            if not (out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and out.dim() == 2 and out.shape[1] == 3):
                raise ValueError("out must be a contiguous int32 CUDA tensor of shape [cap, 3]")
            cap = out.shape[0] if cap is None else min(int(cap), out.shape[0])
        else:
            cap = 0
        if doc_sel_offsets is not None and not (doc_sel_offsets.is_cuda and doc_sel_offsets.dtype in (torch.int64, torch.uint64)
                                                and doc_sel_offsets.is_contiguous()
                                                and doc_sel_offsets.numel() >= doc_offsets.numel()):
            raise ValueError("doc_sel_offsets must be a contiguous int64/uint64 CUDA tensor of at least D + 1 entries")
        D = doc_offsets.numel() - 1
        p = _params(False, sep)
        n, nh = C.c_uint64(0), C.c_uint64(0)
        s = stream if stream is not None else torch.cuda.current_stream(corpus.device).cuda_stream
        rc = N.lib().aha_ac_select_batch_device(
            self._h, corpus.data_ptr(), doc_offsets.data_ptr(), D, corpus.numel(), C.byref(p), flags,
            out.data_ptr() if out is not None and cap else None, cap,
            doc_sel_offsets.data_ptr() if doc_sel_offsets is not None else None, C.byref(n), C.byref(nh), C.c_void_p(s))
        if rc == N.AHA_E_CAPACITY:
            e = AhaError(rc, N.lib().aha_strerror(rc).decode())
            e.n_required = int(n.value)
            raise e
        self._check(rc)
        return int(n.value), int(nh.value)

    def select_corpus(self, corpus, sep=None, flags=0):
        """The selection of a batch that already lives in HBM (DeviceCorpus), downloaded:
        -> (hits HIT_DTYPE, doc_sel_offsets uint64[D+1], n_hits)."""
        D = corpus.n_docs
        p = _params(False, sep)
        dev = corpus.device
        dso = DeviceBuffer(dev, (D + 1) * 8)
        n, nh = C.c_uint64(0), C.c_uint64(0)
        L = N.lib()
        rc = L.aha_ac_select_batch_device(self._h, corpus.ptr, corpus.doc_ptr, D, corpus.n_bytes, C.byref(p), flags, None, 0,
                                          dso.ptr, C.byref(n), C.byref(nh), None)
        if rc != N.AHA_E_CAPACITY:
            self._check(rc)
            return np.zeros(0, dtype=HIT_DTYPE), dso.download(np.zeros(D + 1, dtype=np.uint64)), int(nh.value)
        cap = int(n.value)
        out = DeviceBuffer(dev, cap * 12)
        rc = L.aha_ac_select_batch_device(self._h, corpus.ptr, corpus.doc_ptr, D, corpus.n_bytes, C.byref(p), flags, out.ptr, cap,
                                          dso.ptr, C.byref(n), C.byref(nh), None)
        self._check(rc)
        return (out.download(np.zeros(cap, dtype=HIT_DTYPE)), dso.download(np.zeros(D + 1, dtype=np.uint64)), int(nh.value))

    # -- tokens: dictionary segmentation (forward maximum matching) through the select entries (AHA_SELECT_TOKENS) ----------
    @staticmethod
    def _token_flags(gap_runs):
        return N.AHA_SELECT_TOKENS | (N.AHA_SELECT_GAP_RUNS if gap_runs else 0)

    def tokens_batch(self, corpus, doc_offsets, sep=None, gap_runs=False, cap=None):
        """Every document as a gap-free sequence of tokens: the hits of select_batch(corpus, doc_offsets, sep) with their key
        index as value, and between them one token per character (gap_runs: one per gap) with value -1.  Byte offsets:
        -> (tokens HIT_DTYPE, doc_tok_offsets uint64[D+1]).  cap None: a sizing call first."""
        return self.select_batch(corpus, doc_offsets, sep=sep, cap=cap, flags=self._token_flags(gap_runs))

    def tokens_batch_device(self, corpus, doc_offsets, out, doc_tok_offsets=None, sep=None, gap_runs=False, cap=None, stream=None):
        """Device-resident tokens on torch CUDA tensors, as select_batch_device: out int32 [cap, 3] ({start, end, value} rows;
        column 2 is the id stream, -1 for a token that is no key) or None (a sizing call).  -> (n_tokens, n_hits)."""
        return self.select_batch_device(corpus, doc_offsets, out, doc_sel_offsets=doc_tok_offsets, sep=sep, cap=cap, stream=stream,
                                        flags=self._token_flags(gap_runs))

    def tokens_corpus(self, corpus, sep=None, gap_runs=False):
        """The tokens of a batch that already lives in HBM (DeviceCorpus), downloaded:
        -> (tokens HIT_DTYPE, doc_tok_offsets uint64[D+1], n_hits)."""
        return self.select_corpus(corpus, sep=sep, flags=self._token_flags(gap_runs))

    def tokens(self, seq, sep=None, gap_runs=False):
        """The tokens of one sequence.  bytes in: a list of Hit (byte offsets, value -1 for a token that is no key); str in: a
        list of (text, value) -- the slices are cut from the UTF-8 bytes and decoded, so a key that ends inside a character
        (byte-level keys) gives replacement characters, never an exception."""
        b = _b(seq)
        toks, _ = self.tokens_batch(np.frombuffer(b, dtype=np.uint8), np.array([0, len(b)], dtype=np.uint64), sep=sep,
                                    gap_runs=gap_runs)
        if isinstance(seq, str):
            return [(b[s:e].decode("utf-8", errors="replace"), v) for s, e, v in toks.tolist()]
        return [Hit(s, e, v) for s, e, v in toks.tolist()]

    def segment(self, seq, sep=None, gap_runs=False):
        """Just the pieces of tokens(seq): str in, a list of str; bytes in, a list of bytes."""
        if isinstance(seq, str):
            return [t for t, _ in self.tokens(seq, sep=sep, gap_runs=gap_runs)]
        b = _b(seq)
        return [b[t.start:t.end] for t in self.tokens(b, sep=sep, gap_runs=gap_runs)]

    # -- replace: the substituted copy of a batch, built on the device (aha_ac_replace_batch*) ----------
    def replacements(self, repl):
        """repl -- a mapping from key index to bytes / str / None (keys it does not name are kept) or a sequence with one entry
        per key (None: keep) -- as a ReplTable of this handle."""
        n_keys = self.n_keys
        blob, offs, keep = _pack_replacements(repl, n_keys)
        h = C.c_void_p()
        self._check(N.lib().aha_repl_create(self._h, _ptr(blob), _ptr(offs), _ptr(keep), C.byref(h)))
        t = ReplTable(h, n_keys)
        t._keep_alive = (blob, offs, keep)
        return t

    def _table(self, repl_or_table):
        return repl_or_table if isinstance(repl_or_table, ReplTable) else self.replacements(repl_or_table)

    @staticmethod
    def _capacity_error(rc, n):
        e = AhaError(rc, N.lib().aha_strerror(rc).decode())
        e.n_required = int(n.value)
        return e

    def replace_batch(self, corpus, doc_offsets, repl_or_table, sep=None):
        """Every document with its selected hits (select_batch) replaced as the table says, built on the device:
        -> (uint8 array, doc_out_offsets uint64[D+1]); document d's result is out[doc_out_offsets[d]:doc_out_offsets[d+1]].
        A sizing call first."""
        if isinstance(corpus, (bytes, bytearray)):
            corpus = np.frombuffer(bytes(corpus), dtype=np.uint8)
        corpus = np.ascontiguousarray(corpus, dtype=np.uint8)
        doc_offsets = np.ascontiguousarray(doc_offsets, dtype=np.uint64)
        table = self._table(repl_or_table)
        D = doc_offsets.size - 1
        p = _params(False, sep)
        doo = np.zeros(D + 1, dtype=np.uint64)
        n = C.c_uint64(0)
        L = N.lib()
        rc = L.aha_ac_replace_batch(self._h, table._h, _ptr(corpus), _ptr(doc_offsets), D, C.byref(p), 0, None, 0, _ptr(doo),
                                    C.byref(n), None, None)
        if rc != N.AHA_E_CAPACITY:
            self._check(rc)
            return np.zeros(0, dtype=np.uint8), doo
        cap = int(n.value)
        out = np.zeros(cap, dtype=np.uint8)
        rc = L.aha_ac_replace_batch(self._h, table._h, _ptr(corpus), _ptr(doc_offsets), D, C.byref(p), 0, _ptr(out), cap,
                                    _ptr(doo), C.byref(n), None, None)
        self._check(rc)
        return out[: int(n.value)], doo

    def replace_batch_device(self, corpus, doc_offsets, table, out, doc_out_offsets=None, sep=None, cap=None, stream=None):
        """Device-resident replace on torch CUDA tensors: uint8 corpus, int64/uint64 doc offsets, out uint8 [cap] (any
        alignment) or None (a sizing call), doc_out_offsets int64/uint64 [D+1] or None.
        -> (n_out_bytes, n_selected, n_hits); raises AhaError(AHA_E_CAPACITY) when out is too small (e.n_required = the bytes
        needed); nothing is written then."""
        import torch

        assert corpus.is_cuda and corpus.dtype == torch.uint8 and corpus.is_contiguous()
        assert doc_offsets.is_cuda and doc_offsets.dtype in (torch.int64, torch.uint64)
        if out is not None:
            if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.dim() == 1):
                raise ValueError("out must be a contiguous one-dimensional uint8 CUDA tensor")
            cap = out.numel() if cap is None else min(int(cap), out.numel())
        else:
            cap = 0
        if doc_out_offsets is not None and not (doc_out_offsets.is_cuda and doc_out_offsets.dtype in (torch.int64, torch.uint64)
                                                and doc_out_offsets.is_contiguous()
                                                and doc_out_offsets.numel() >= doc_offsets.numel()):
            raise ValueError("doc_out_offsets must be a contiguous int64/uint64 CUDA tensor of at least D + 1 entries")
        D = doc_offsets.numel() - 1
        p = _params(False, sep)
        n, ns, nh = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        s = stream if stream is not None else torch.cuda.current_stream(corpus.device).cuda_stream
        rc = N.lib().aha_ac_replace_batch_device(
            self._h, table._h, corpus.data_ptr(), doc_offsets.data_ptr(), D, corpus.numel(), C.byref(p), 0,
            out.data_ptr() if out is not None and cap else None, cap,
            doc_out_offsets.data_ptr() if doc_out_offsets is not None else None, C.byref(n), C.byref(ns), C.byref(nh),
            C.c_void_p(s))
        if rc == N.AHA_E_CAPACITY:
            raise self._capacity_error(rc, n)
        self._check(rc)
        return int(n.value), int(ns.value), int(nh.value)

    def replace_corpus(self, corpus, table, sep=None):
        """The substituted copy of a batch that already lives in HBM (DeviceCorpus), downloaded:
        -> (uint8 array, doc_out_offsets uint64[D+1], n_selected, n_hits)."""
        table = self._table(table)
        D = corpus.n_docs
        p = _params(False, sep)
        dev = corpus.device
        doo = DeviceBuffer(dev, (D + 1) * 8)
        n, ns, nh = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        L = N.lib()
        rc = L.aha_ac_replace_batch_device(self._h, table._h, corpus.ptr, corpus.doc_ptr, D, corpus.n_bytes, C.byref(p), 0, None, 0,
                                           doo.ptr, C.byref(n), C.byref(ns), C.byref(nh), None)
        if rc != N.AHA_E_CAPACITY:
            self._check(rc)
            return (np.zeros(0, dtype=np.uint8), doo.download(np.zeros(D + 1, dtype=np.uint64)), int(ns.value), int(nh.value))
        cap = int(n.value)
        out = DeviceBuffer(dev, cap)
        rc = L.aha_ac_replace_batch_device(self._h, table._h, corpus.ptr, corpus.doc_ptr, D, corpus.n_bytes, C.byref(p), 0, out.ptr,
                                           cap, doo.ptr, C.byref(n), C.byref(ns), C.byref(nh), None)
        self._check(rc)
        return (out.download(np.zeros(cap, dtype=np.uint8)), doo.download(np.zeros(D + 1, dtype=np.uint64)), int(ns.value),
                int(nh.value))

    # -- class counts: hits per key class within each document, dense (aha_ac_class_counts_batch*) ----------
    def classes(self, spec, n_classes=None):
        """A Classes table of this handle from spec:
        a sequence of K items, one per key -- None (no class), an int, or a sequence of ints;
        or a mapping {class: iterable of keys} where a class is an int id or a name (names become the columns in the mapping's
        order, kept as Classes.names) and a key is its index or its spelling (bytes / str).
        n_classes: C where it is more than the largest id + 1."""
        K = self.n_keys
        per_key = [set() for _ in range(K)]
        names = None
        if hasattr(spec, "keys"):
            labels = list(spec.keys())
            by_name = not all(isinstance(c, (int, np.integer)) and not isinstance(c, bool) for c in labels)
            if by_name:
                names = labels
            for col, label in enumerate(labels):
                c = col if by_name else int(label)
                for key in spec[label]:
                    k = int(key) if isinstance(key, (int, np.integer)) else self[key]
                    if not 0 <= k < K:
                        raise ValueError("the class table names key %r; the handle has %d keys" % (key, K))
                    per_key[k].add(c)
        else:
            if len(spec) != K:
                raise ValueError("the class table must have one entry per key (%d), or be a mapping from class to keys" % K)
            for k, item in enumerate(spec):
                if item is None:
                    continue
                per_key[k].update([int(item)] if isinstance(item, (int, np.integer)) else [int(c) for c in item])
        top = max((max(cs) for cs in per_key if cs), default=-1)
        low = min((min(cs) for cs in per_key if cs), default=0)
        if low < 0:
            raise ValueError("class ids are not negative")
        C_ = max(top + 1, len(names) if names else 0, 1) if n_classes is None else int(n_classes)
        offs = np.zeros(K + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(cs) for cs in per_key])
        ids = np.array([c for cs in per_key for c in sorted(cs)], dtype=np.uint32)
        h = C.c_void_p()
        self._check(N.lib().aha_classes_create(self._h, _ptr(ids), _ptr(offs), C_, C.byref(h)))
        return Classes(h, K, C_, names)

    def _classes(self, classes):
        return classes if isinstance(classes, Classes) else self.classes(classes)

    def class_counts_batch(self, corpus, doc_offsets, classes, sep=None):
        """Per document the hits of match_batch(corpus, doc_offsets, sep) counted by key class: -> uint32 array of shape
        (D, C); entry [d, c] = the hits of document d whose key is in class c (a key in several classes counts in each)."""
        if isinstance(corpus, (bytes, bytearray)):
            corpus = np.frombuffer(bytes(corpus), dtype=np.uint8)
        corpus = np.ascontiguousarray(corpus, dtype=np.uint8)
        doc_offsets = np.ascontiguousarray(doc_offsets, dtype=np.uint64)
        table = self._classes(classes)
        D = doc_offsets.size - 1
        p = _params(False, sep)
        out = np.zeros((D, table.n_classes), dtype=np.uint32)
        self._check(N.lib().aha_ac_class_counts_batch(self._h, table._h, _ptr(corpus), _ptr(doc_offsets), D, C.byref(p), 0,
                                                      _ptr(out), None))
        return out

    def class_counts(self, seq, classes, sep=None):
        """The hits of match(seq, sep) counted by key class: -> uint32[C]."""
        b = _b(seq)
        return self.class_counts_batch(np.frombuffer(b, dtype=np.uint8), np.array([0, len(b)], dtype=np.uint64), classes, sep=sep)[0]

    def class_counts_batch_device(self, corpus, doc_offsets, classes, out, sep=None, stream=None):
        """Device-resident class counts on torch CUDA tensors: uint8 corpus, int64/uint64 doc offsets, out a contiguous int32
        tensor of shape (D, C), every entry of which is written (as uint32).  -> n_hits."""
        import torch

        assert corpus.is_cuda and corpus.dtype == torch.uint8 and corpus.is_contiguous()
        assert doc_offsets.is_cuda and doc_offsets.dtype in (torch.int64, torch.uint64)
        D = doc_offsets.numel() - 1
        if not (out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and tuple(out.shape) == (D, classes.n_classes)):
            raise ValueError("out must be a contiguous int32 CUDA tensor of shape (D, C) = (%d, %d)" % (D, classes.n_classes))
        p = _params(False, sep)
        nh = C.c_uint64(0)
        s = stream if stream is not None else torch.cuda.current_stream(corpus.device).cuda_stream
        self._check(N.lib().aha_ac_class_counts_batch_device(
            self._h, classes._h, corpus.data_ptr(), doc_offsets.data_ptr(), D, corpus.numel(), C.byref(p), 0,
            out.data_ptr() if D else None, C.byref(nh), C.c_void_p(s)))
        return int(nh.value)

    def class_counts_corpus(self, corpus, classes, sep=None):
        """The class counts of a batch that already lives in HBM (DeviceCorpus), downloaded: -> (uint32 (D, C), n_hits)."""
        table = self._classes(classes)
        D, C_ = corpus.n_docs, table.n_classes
        p = _params(False, sep)
        out = DeviceBuffer(corpus.device, max(D * C_ * 4, 4))
        nh = C.c_uint64(0)
        self._check(N.lib().aha_ac_class_counts_batch_device(self._h, table._h, corpus.ptr, corpus.doc_ptr, D, corpus.n_bytes,
                                                             C.byref(p), 0, out.ptr, C.byref(nh), None))
        return out.download(np.zeros((D, C_), dtype=np.uint32)), int(nh.value)

    # -- rule grep: keep documents by conditions on their class counts (aha_ac_grep_batch* with AHA_GREP_RULE) ----
    def rule(self, spec, classes):
        """A Rule over the class counts of `classes` (a Classes of this handle, or what AC.classes takes) from spec: a list
        of groups, a group a list of terms (class, ">=" | "<", num) or (class, op, num, per_bytes); a class is its index, or
        its name where the Classes has names.  (c, ">=", 3) is "at least 3 hits of class c"; (c, ">=", 3, 1000) is "at
        least 3 hits of class c per 1000 bytes of the document".  A document passes when some group has all its terms
        true.  1 to 64 terms in all; ValueError otherwise."""
        table = self._classes(classes)
        ops = {">=": N.AHA_RULE_GE, "<": N.AHA_RULE_LT}
        terms = []
        groups = list(spec)
        for g, group in enumerate(groups):
            if isinstance(group, tuple) or not hasattr(group, "__iter__") or isinstance(group, (str, bytes)):
                raise ValueError("a rule is a list of groups, a group a list of terms")
            group = list(group)
            if not group:
                raise ValueError("group %d of the rule has no term" % g)
            for term in group:
                if len(term) not in (3, 4):
                    raise ValueError("a term is (class, op, num) or (class, op, num, per_bytes): %r" % (term,))
                c, op, num = term[0], term[1], term[2]
                den = term[3] if len(term) == 4 else 0
                if op not in ops:
                    raise ValueError("a term's op is '>=' or '<': %r" % (op,))
                if isinstance(c, (int, np.integer)) and not isinstance(c, bool):
                    c = int(c)
                elif table.names is not None and c in table.names:
                    c = table.names.index(c)
                else:
                    raise ValueError("the rule names class %r; the table has %s" % (c, table.names or "no names"))
                if not 0 <= c < table.n_classes:
                    raise ValueError("the rule names class %d; the table has %d classes" % (c, table.n_classes))
                num, den = int(num), int(den)
                if not (0 <= num < 1 << 32 and 0 <= den < 1 << 32):
                    raise ValueError("num and per_bytes are 32-bit and not negative: %r" % (term,))
                terms.append((c, ops[op], g, num, den))
        if not 1 <= len(terms) <= N.AHA_RULE_MAX_TERMS:
            raise ValueError("a rule has 1 to %d terms, this one %d" % (N.AHA_RULE_MAX_TERMS, len(terms)))
        return Rule(table, terms)

    def _grep_params(self, sep, invert, classes, rule, rows_ptr):
        """-> (params pointer, flags, what must stay alive over the call, the Classes or None) of a grep call"""
        flags = N.AHA_GREP_INVERT if invert else 0
        if rule is None:
            if classes is not None or rows_ptr is not None:
                raise ValueError("classes and rows belong to a rule: give rule=")
            p = _params(False, sep)
            return C.pointer(p), flags, p, None
        if not isinstance(rule, Rule):
            if classes is None:
                raise ValueError("a rule given as a spec needs classes=")
            rule = self.rule(rule, classes)
        elif classes is not None and classes is not rule.classes:
            raise ValueError("the rule was made for another Classes")
        gp = N.aha_grep_params()
        gp.match = _params(False, sep)
        gp.match.struct_size = C.sizeof(N.aha_grep_params)
        gp.classes = rule.classes._h
        gp.terms = C.cast(rule._arr, C.POINTER(N.aha_rule_term))
        gp.n_terms = len(rule.terms)
        gp.reserved = 0
        gp.rows = rows_ptr
        return C.cast(C.pointer(gp), C.POINTER(N.aha_match_params)), flags | N.AHA_GREP_RULE, (gp, rule), rule.classes

    # -- context lines: the records around a matching record (aha_ac_grep_batch* with AHA_GREP_LINES) -------------------------
    @staticmethod
    def _lines_spec(before, after, context, groups, matched, rule):
        """-> None where none of the context keywords is given (the call is plain grep's), else (before, after); checked
        before the library is called"""
        plain = lambda v: not isinstance(v, bool) and isinstance(v, (int, np.integer)) and int(v) == 0
        if context is None and groups is None and matched is None and plain(before) and plain(after):
            return None
        if rule is not None:
            raise ValueError("before, after, context, groups and matched do not combine with rule=")
        if context is not None:
            if not (plain(before) and plain(after)):
                raise ValueError("context sets both sides: give it, or before and after")
            before = after = context
        for name, v in (("before", before), ("after", after)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError("%s is a record count: %r" % (name, v))
            if not 0 <= int(v) <= 0x7FFFFFFF:
                raise ValueError("%s is 0 .. 0x7FFFFFFF: %r" % (name, v))
        return int(before), int(after)

    @staticmethod
    def _lines_params(sep, invert, spec, groups_ptr, n_groups):
        """-> (params pointer, flags, the aha_grep_lines_params: it must stay alive over the call, is_match is set on it)"""
        lp = N.aha_grep_lines_params()
        lp.match = _params(False, sep)
        lp.match.struct_size = C.sizeof(N.aha_grep_lines_params)
        lp.before, lp.after, lp.flags, lp.reserved = spec[0], spec[1], 0, 0
        lp.group_offsets, lp.n_groups, lp.is_match = (groups_ptr, n_groups, None) if n_groups else (None, 0, None)
        flags = N.AHA_GREP_LINES | (N.AHA_GREP_INVERT if invert else 0)
        return C.cast(C.pointer(lp), C.POINTER(N.aha_match_params)), flags, lp

    @staticmethod
    def _host_groups(groups):
        """groups of a host call -> a contiguous uint64 array of G + 1 entries, or None"""
        if groups is None:
            return None
        g = np.ascontiguousarray(groups, dtype=np.uint64)
        if g.ndim != 1 or g.size < 1:
            raise ValueError("groups is a one-dimensional array of G + 1 record offsets")
        return g

    @staticmethod
    def _host_matched(matched):
        if matched is None:
            return None
        if not (isinstance(matched, np.ndarray) and matched.dtype == np.uint8 and matched.ndim == 1 and matched.flags.c_contiguous
                and matched.flags.writeable):
            raise ValueError("matched must be a contiguous writeable one-dimensional uint8 array")
        return matched

    @staticmethod
    def _host_rows(rows, D, table):
        if rows is None:
            return None
        if not (isinstance(rows, np.ndarray) and rows.dtype == np.uint32 and rows.flags.c_contiguous and rows.flags.writeable
                and rows.shape == (D, table.n_classes)):
            raise ValueError("rows must be a contiguous uint32 array of shape (D, C) = (%d, %d)" % (D, table.n_classes))
        return rows

    # -- records and grep: split a batch into records, keep those with a hit (aha_ac_records_batch*, aha_ac_grep_batch*) ----
    def records(self, corpus, doc_offsets=None, delim=b"\n"):
        """The batch split into records at the delimiter byte and at the documents' ends, on the device:
        -> (rec_offsets uint64[R+1], doc_rec_offsets uint64[D+1]).  A record ends behind a delimiter or at a document's end
        and is never empty; document d's records are rec_offsets[doc_rec_offsets[d]:doc_rec_offsets[d+1] + 1].  rec_offsets
        is a doc_offsets for every batch call.  doc_offsets None: the corpus is one document.  A sizing call first."""
        if isinstance(corpus, (bytes, bytearray)):
            corpus = np.frombuffer(bytes(corpus), dtype=np.uint8)
        corpus = np.ascontiguousarray(corpus, dtype=np.uint8)
        if doc_offsets is None:
            doc_offsets = [0, corpus.size]
        doc_offsets = np.ascontiguousarray(doc_offsets, dtype=np.uint64)
        D = doc_offsets.size - 1
        dro = np.zeros(D + 1, dtype=np.uint64)
        n = C.c_uint64(0)
        L = N.lib()
        d = _delim_byte(delim)
        rc = L.aha_ac_records_batch(self._h, _ptr(corpus), _ptr(doc_offsets), D, d, 0, None, 0, None, C.byref(n))
        if rc != N.AHA_E_CAPACITY:
            self._check(rc)
        cap = int(n.value)
        rec = np.zeros(cap + 1, dtype=np.uint64)
        self._check(L.aha_ac_records_batch(self._h, _ptr(corpus), _ptr(doc_offsets), D, d, 0, _ptr(rec), cap, _ptr(dro), C.byref(n)))
        return rec[: int(n.value) + 1], dro

    def records_device(self, corpus, doc_offsets, rec_offsets, doc_rec_offsets=None, delim=b"\n", cap=None, stream=None):
        """Device-resident records on torch CUDA tensors: uint8 corpus (any alignment), int64/uint64 doc offsets, rec_offsets
        int64/uint64 [cap + 1] or None (a sizing call), doc_rec_offsets int64/uint64 [D+1] or None.
        -> n_records; raises AhaError(AHA_E_CAPACITY) when rec_offsets is too small (e.n_required = the records needed);
        nothing is written then."""
        import torch

        assert corpus.is_cuda and corpus.dtype == torch.uint8 and corpus.is_contiguous()
        assert doc_offsets.is_cuda and doc_offsets.dtype in (torch.int64, torch.uint64)
        if rec_offsets is not None:
            if not (rec_offsets.is_cuda and rec_offsets.dtype in (torch.int64, torch.uint64) and rec_offsets.is_contiguous()
                    and rec_offsets.numel() >= 1):
                raise ValueError("rec_offsets must be a contiguous int64/uint64 CUDA tensor of at least one entry")
            cap = rec_offsets.numel() - 1 if cap is None else min(int(cap), rec_offsets.numel() - 1)
        else:
            cap = 0
        if doc_rec_offsets is not None and not (doc_rec_offsets.is_cuda and doc_rec_offsets.dtype in (torch.int64, torch.uint64)
                                                and doc_rec_offsets.is_contiguous()
                                                and doc_rec_offsets.numel() >= doc_offsets.numel()):
            raise ValueError("doc_rec_offsets must be a contiguous int64/uint64 CUDA tensor of at least D + 1 entries")
        D = doc_offsets.numel() - 1
        n = C.c_uint64(0)
        s = stream if stream is not None else torch.cuda.current_stream(corpus.device).cuda_stream
        rc = N.lib().aha_ac_records_batch_device(
            self._h, corpus.data_ptr(), doc_offsets.data_ptr(), D, corpus.numel(), _delim_byte(delim), 0,
            rec_offsets.data_ptr() if rec_offsets is not None else None, cap,
            doc_rec_offsets.data_ptr() if doc_rec_offsets is not None else None, C.byref(n), C.c_void_p(s))
        if rc == N.AHA_E_CAPACITY:
            raise self._capacity_error(rc, n)
        self._check(rc)
        return int(n.value)

    @staticmethod
    def _grep_capacity_error(rc, n_docs, n_bytes):
        e = AhaError(rc, N.lib().aha_strerror(rc).decode())
        e.n_required = int(n_docs.value)
        e.bytes_required = int(n_bytes.value)
        return e

    def grep_batch(self, corpus, doc_offsets, sep=None, invert=False, text=True, classes=None, rule=None, rows=None, before=0,
                   after=0, context=None, groups=None, matched=None):
        """The documents with at least one hit of match_batch(corpus, doc_offsets, sep) -- invert: those without one --
        compacted on the device: -> (kept_docs uint64[n_kept], uint8 array, doc_out_offsets uint64[n_kept+1]); kept document
        i is document kept_docs[i] and its bytes are out[doc_out_offsets[i]:doc_out_offsets[i+1]].  text False: no bytes are
        copied (an empty array comes back).  A sizing call first.
        rule (a Rule of AC.rule, or its spec with classes=): the documents whose class counts pass the rule instead -- invert:
        those that do not; rows (a uint32 array of shape (D, C)) then receives class_counts_batch of the batch.
        before, after (context: both): grep -B, -A, -C -- that many documents (records) in front of and behind a matching one
        are kept with it, inside the groups (uint64[G + 1] offsets into the documents, such as records()'s doc_rec_offsets;
        None: one group); matched (a uint8 array of at least n_kept entries) receives 1 where the kept document matched, 0
        where it is context.  Not with rule=."""
        spec = self._lines_spec(before, after, context, groups, matched, rule)
        if isinstance(corpus, (bytes, bytearray)):
            corpus = np.frombuffer(bytes(corpus), dtype=np.uint8)
        corpus = np.ascontiguousarray(corpus, dtype=np.uint8)
        doc_offsets = np.ascontiguousarray(doc_offsets, dtype=np.uint64)
        D = doc_offsets.size - 1
        if spec is not None:
            if classes is not None or rows is not None:
                raise ValueError("classes and rows belong to a rule: give rule=")
            return self._grep_lines_host(corpus, doc_offsets, D, sep, invert, text, spec, groups, matched)
        p, flags, _alive, table = self._grep_params(sep, invert, classes, rule, None)
        if rows is not None:
            if table is None:
                raise ValueError("classes and rows belong to a rule: give rule=")
            rows = self._host_rows(rows, D, table)
        nk, nb = C.c_uint64(0), C.c_uint64(0)
        L = N.lib()
        self._check(L.aha_ac_grep_batch(self._h, _ptr(corpus), _ptr(doc_offsets), D, p, flags, None, None, 0, None, 0,
                                        C.byref(nk), C.byref(nb), None))
        cap_docs, cap_bytes = int(nk.value), int(nb.value) if text else 0
        kept = np.zeros(max(cap_docs, 1), dtype=np.uint64)
        doo = np.zeros(cap_docs + 1, dtype=np.uint64)
        out = np.zeros(max(cap_bytes, 1), dtype=np.uint8)
        if rows is not None and rows.size:
            _alive[0].rows = rows.ctypes.data
        self._check(L.aha_ac_grep_batch(self._h, _ptr(corpus), _ptr(doc_offsets), D, p, flags, _ptr(kept), _ptr(doo),
                                        cap_docs, _ptr(out) if text else None, cap_bytes, C.byref(nk), C.byref(nb), None))
        return kept[: int(nk.value)], out[: int(nb.value) if text else 0], doo[: int(nk.value) + 1]

    def _grep_lines_host(self, corpus, doc_offsets, D, sep, invert, text, spec, groups, matched):
        """grep_batch with context lines: the same two calls, the second with is_match where matched was given"""
        g = self._host_groups(groups)
        matched = self._host_matched(matched)
        p, flags, lp = self._lines_params(sep, invert, spec, g.ctypes.data if g is not None else None, g.size - 1 if g is not None else 0)
        nk, nb = C.c_uint64(0), C.c_uint64(0)
        L = N.lib()
        self._check(L.aha_ac_grep_batch(self._h, _ptr(corpus), _ptr(doc_offsets), D, p, flags, None, None, 0, None, 0,
                                        C.byref(nk), C.byref(nb), None))
        cap_docs, cap_bytes = int(nk.value), int(nb.value) if text else 0
        if matched is not None and matched.size < cap_docs:
            raise ValueError("matched has %d entries, the call keeps %d documents" % (matched.size, cap_docs))
        kept = np.zeros(max(cap_docs, 1), dtype=np.uint64)
        doo = np.zeros(cap_docs + 1, dtype=np.uint64)
        out = np.zeros(max(cap_bytes, 1), dtype=np.uint8)
        if matched is not None and cap_docs:
            lp.is_match = matched.ctypes.data
        self._check(L.aha_ac_grep_batch(self._h, _ptr(corpus), _ptr(doc_offsets), D, p, flags, _ptr(kept), _ptr(doo),
                                        cap_docs, _ptr(out) if text else None, cap_bytes, C.byref(nk), C.byref(nb), None))
        return kept[: int(nk.value)], out[: int(nb.value) if text else 0], doo[: int(nk.value) + 1]

    def grep_batch_device(self, corpus, doc_offsets, kept_docs=None, doc_out_offsets=None, out=None, sep=None, invert=False,
                          cap_docs=None, cap_bytes=None, stream=None, classes=None, rule=None, rows=None, before=0, after=0,
                          context=None, groups=None, matched=None):
        """Device-resident grep on torch CUDA tensors: uint8 corpus, int64/uint64 doc offsets, kept_docs int64/uint64
        [cap_docs] or None, doc_out_offsets int64/uint64 [cap_docs + 1] or None, out uint8 [cap_bytes] (any alignment) or None
        (no bytes are copied).  -> (n_kept, n_out_bytes, n_hits); raises AhaError(AHA_E_CAPACITY) when a buffer is too small
        (e.n_required = the documents needed, e.bytes_required = the bytes needed); nothing is written then.
        rule (a Rule of AC.rule, or its spec with classes=): the documents whose class counts pass the rule; rows: a
        contiguous int32 CUDA tensor of shape (D, C) that receives the class counts (as uint32), as class_counts_batch_device
        writes them.
        before, after, context: as in grep_batch; groups: an int64/uint64 CUDA tensor of G + 1 record offsets (such as
        records_device's doc_rec_offsets) or None; matched: a uint8 CUDA tensor that receives 1 where the kept document
        matched and 0 where it is context (it bounds cap_docs as kept_docs does).  Not with rule=."""
        import torch

        spec = self._lines_spec(before, after, context, groups, matched, rule)
        if spec is not None and (classes is not None or rows is not None):
            raise ValueError("classes and rows belong to a rule: give rule=")
        assert corpus.is_cuda and corpus.dtype == torch.uint8 and corpus.is_contiguous()
        assert doc_offsets.is_cuda and doc_offsets.dtype in (torch.int64, torch.uint64)
        for name, t in (("kept_docs", kept_docs), ("doc_out_offsets", doc_out_offsets), ("groups", groups)):
            if t is not None and not (t.is_cuda and t.dtype in (torch.int64, torch.uint64) and t.is_contiguous()):
                raise ValueError(name + " must be a contiguous int64/uint64 CUDA tensor")
        if groups is not None and (groups.dim() != 1 or groups.numel() < 1):
            raise ValueError("groups is a one-dimensional tensor of G + 1 record offsets")
        if matched is not None and not (matched.is_cuda and matched.dtype == torch.uint8 and matched.is_contiguous()
                                        and matched.dim() == 1):
            raise ValueError("matched must be a contiguous one-dimensional uint8 CUDA tensor")
        room = []
        if matched is not None:
            room.append(matched.numel())
        if kept_docs is not None:
            room.append(kept_docs.numel())
        if doc_out_offsets is not None:
            if doc_out_offsets.numel() < 1:
                raise ValueError("doc_out_offsets must have at least one entry")
            room.append(doc_out_offsets.numel() - 1)
        cap_docs = 0 if not room else min(room) if cap_docs is None else min([int(cap_docs)] + room)
        if out is not None:
            if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.dim() == 1):
                raise ValueError("out must be a contiguous one-dimensional uint8 CUDA tensor")
            cap_bytes = out.numel() if cap_bytes is None else min(int(cap_bytes), out.numel())
        else:
            cap_bytes = 0
        D = doc_offsets.numel() - 1
        if spec is not None:
            p, flags, _alive = self._lines_params(sep, invert, spec, groups.data_ptr() if groups is not None else None,
                                                  groups.numel() - 1 if groups is not None else 0)
            if matched is not None and cap_docs:
                _alive.is_match = matched.data_ptr()
            table = None
        else:
            p, flags, _alive, table = self._grep_params(sep, invert, classes, rule, None)
        if rows is not None:
            if table is None:
                raise ValueError("classes and rows belong to a rule: give rule=")
            if not (rows.is_cuda and rows.dtype == torch.int32 and rows.is_contiguous() and tuple(rows.shape) == (D, table.n_classes)):
                raise ValueError("rows must be a contiguous int32 CUDA tensor of shape (D, C) = (%d, %d)" % (D, table.n_classes))
            if D:
                _alive[0].rows = rows.data_ptr()
        nk, nb, nh = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        s = stream if stream is not None else torch.cuda.current_stream(corpus.device).cuda_stream
        rc = N.lib().aha_ac_grep_batch_device(
            self._h, corpus.data_ptr(), doc_offsets.data_ptr(), D, corpus.numel(), p, flags,
            kept_docs.data_ptr() if kept_docs is not None else None,
            doc_out_offsets.data_ptr() if doc_out_offsets is not None else None, cap_docs,
            out.data_ptr() if out is not None else None, cap_bytes, C.byref(nk), C.byref(nb), C.byref(nh), C.c_void_p(s))
        if rc == N.AHA_E_CAPACITY:
            raise self._grep_capacity_error(rc, nk, nb)
        self._check(rc)
        return int(nk.value), int(nb.value), int(nh.value)

    def grep_corpus(self, corpus, sep=None, invert=False, text=True, classes=None, rule=None, rows=None, before=0, after=0,
                    context=None, groups=None, matched=None):
        """grep_batch of a batch that already lives in HBM (DeviceCorpus), downloaded:
        -> (kept_docs uint64[n_kept], uint8 array, doc_out_offsets uint64[n_kept+1], n_hits).  rule, classes, rows: as in
        grep_batch (rows a uint32 array of shape (D, C), downloaded into).  before, after, context, groups, matched: as in
        grep_batch (groups a host array, uploaded; matched a host array, downloaded into)."""
        spec = self._lines_spec(before, after, context, groups, matched, rule)
        D = corpus.n_docs
        dev = corpus.device
        d_groups = d_matched = None
        if spec is not None:
            if classes is not None or rows is not None:
                raise ValueError("classes and rows belong to a rule: give rule=")
            g = self._host_groups(groups)
            matched = self._host_matched(matched)
            if g is not None and g.size > 1:
                d_groups = DeviceBuffer(dev, g.nbytes)
                d_groups.upload(g)
            p, flags, _alive = self._lines_params(sep, invert, spec, d_groups.ptr if d_groups is not None else None,
                                                  g.size - 1 if g is not None else 0)
            table = None
        else:
            p, flags, _alive, table = self._grep_params(sep, invert, classes, rule, None)
        if rows is not None:
            if table is None:
                raise ValueError("classes and rows belong to a rule: give rule=")
            rows = self._host_rows(rows, D, table)
        nk, nb, nh = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        L = N.lib()
        self._check(L.aha_ac_grep_batch_device(self._h, corpus.ptr, corpus.doc_ptr, D, corpus.n_bytes, p, flags, None, None,
                                               0, None, 0, C.byref(nk), C.byref(nb), C.byref(nh), None))
        cap_docs, cap_bytes = int(nk.value), int(nb.value) if text else 0
        kept, doo = DeviceBuffer(dev, max(cap_docs, 1) * 8), DeviceBuffer(dev, (cap_docs + 1) * 8)
        out = DeviceBuffer(dev, max(cap_bytes, 1)) if text else None
        d_rows = DeviceBuffer(dev, rows.size * 4) if rows is not None and rows.size else None
        if d_rows is not None:
            _alive[0].rows = d_rows.ptr
        if spec is not None and matched is not None:
            if matched.size < cap_docs:
                raise ValueError("matched has %d entries, the call keeps %d documents" % (matched.size, cap_docs))
            if cap_docs:
                d_matched = DeviceBuffer(dev, cap_docs)
                _alive.is_match = d_matched.ptr
        self._check(L.aha_ac_grep_batch_device(self._h, corpus.ptr, corpus.doc_ptr, D, corpus.n_bytes, p, flags, kept.ptr,
                                               doo.ptr, cap_docs, out.ptr if text else None, cap_bytes, C.byref(nk), C.byref(nb),
                                               C.byref(nh), None))
        if d_rows is not None:
            d_rows.download(rows)
        if d_matched is not None:
            d_matched.download(matched[:cap_docs])
        got = out.download(np.zeros(max(cap_bytes, 1), dtype=np.uint8))[:cap_bytes] if text else np.zeros(0, dtype=np.uint8)
        return (kept.download(np.zeros(max(cap_docs, 1), dtype=np.uint64))[:cap_docs], got,
                doo.download(np.zeros(cap_docs + 1, dtype=np.uint64)), int(nh.value))

    def grep(self, seq, delim="\n", invert=False, sep=None, classes=None, rule=None, rows=None, before=0, after=0, context=None,
             groups=None, matched=None, separator=None):
        """The records of seq -- split at delim, each with its delimiter -- that have a hit of match(record, sep), as a
        list; invert: those that have none.  bytes in, bytes out; str in, str out.  records plus grep_batch.  rule, classes,
        rows: as in grep_batch, over the records (rows has one row per record of AC.records(seq, None, delim)).
        before, after, context, groups, matched: as in grep_batch, over the records -- grep -B, -A, -C.  separator (a str or
        bytes such as "--\\n"; None: nothing) is inserted as an entry of its own between two kept records that are not
        neighbours or lie in different groups."""
        spec = self._lines_spec(before, after, context, groups, matched, rule)
        b = _b(seq)
        corpus = np.frombuffer(b, dtype=np.uint8)
        rec, _ = self.records(corpus, None, delim)
        if spec is None:
            _, out, doo = self.grep_batch(corpus, rec, sep=sep, invert=invert, classes=classes, rule=rule, rows=rows)
            kept = None
        else:
            kept, out, doo = self.grep_batch(corpus, rec, sep=sep, invert=invert, classes=classes, rows=rows, before=spec[0],
                                             after=spec[1], groups=groups, matched=matched)
        raw = out.tobytes()
        parts = [raw[int(doo[i]):int(doo[i + 1])] for i in range(doo.size - 1)]
        if separator is not None and kept is not None and kept.size > 1:
            g = self._host_groups(groups)
            own = np.searchsorted(g, kept, side="right") if g is not None else np.zeros(kept.size, dtype=np.int64)
            cut = (kept[1:] != kept[:-1] + 1) | (own[1:] != own[:-1])
            mark = _b(separator)
            parts = [x for i, part in enumerate(parts) for x in ((mark, part) if i and cut[i - 1] else (part,))]
        return [x.decode("utf-8") for x in parts] if isinstance(seq, str) else parts

    # -- excerpts: the text around every hit, cut out on the device (aha_ac_grep_batch* with AHA_GREP_CONTEXT) --------------
    @staticmethod
    def _excerpt_params(before, after, sep):
        """-> (params pointer, what must stay alive over the call); the contexts are checked before the library is called"""
        after = before if after is None else after
        for name, v in (("before", before), ("after", after)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError("%s is a byte count: %r" % (name, v))
            if not 0 <= int(v) <= 0x7FFFFFFF:
                raise ValueError("%s is 0 .. 0x7FFFFFFF: %r" % (name, v))
        ep = N.aha_excerpt_params()
        ep.match = _params(False, sep)
        ep.match.struct_size = C.sizeof(N.aha_excerpt_params)
        ep.before, ep.after, ep.flags, ep.reserved = int(before), int(after), 0, 0
        return C.cast(C.pointer(ep), C.POINTER(N.aha_match_params)), ep

    def excerpts_batch(self, corpus, doc_offsets, before, after=None, sep=None, text=True):
        """The hits of match_batch(corpus, doc_offsets, sep) in their context: `before` bytes in front of every hit and `after`
        (None: before) behind it, clipped to the document, snapped outwards to UTF-8 character boundaries, neighbouring
        contexts of one document merged: -> (starts uint64[R], uint8 array, out_offsets uint64[R+1], doc_excerpt_offsets
        uint64[D+1]).  Excerpt r starts at corpus byte starts[r], its bytes are out[out_offsets[r]:out_offsets[r+1]]; document
        d's excerpts are doc_excerpt_offsets[d]:doc_excerpt_offsets[d+1].  text False: no bytes are copied.  A sizing call
        first."""
        p, _alive = self._excerpt_params(before, after, sep)
        if isinstance(corpus, (bytes, bytearray)):
            corpus = np.frombuffer(bytes(corpus), dtype=np.uint8)
        corpus = np.ascontiguousarray(corpus, dtype=np.uint8)
        doc_offsets = np.ascontiguousarray(doc_offsets, dtype=np.uint64)
        D = doc_offsets.size - 1
        nk, nb = C.c_uint64(0), C.c_uint64(0)
        L = N.lib()
        flags = N.AHA_GREP_CONTEXT
        self._check(L.aha_ac_grep_batch(self._h, _ptr(corpus), _ptr(doc_offsets), D, p, flags, None, None, 0, None, 0,
                                        C.byref(nk), C.byref(nb), None))
        cap, cap_bytes = int(nk.value), int(nb.value) if text else 0
        starts = np.zeros(max(cap, 1), dtype=np.uint64)
        oo = np.zeros(cap + 1, dtype=np.uint64)
        out = np.zeros(max(cap_bytes, 1), dtype=np.uint8)
        self._check(L.aha_ac_grep_batch(self._h, _ptr(corpus), _ptr(doc_offsets), D, p, flags, _ptr(starts), _ptr(oo), cap,
                                        _ptr(out) if text else None, cap_bytes, C.byref(nk), C.byref(nb), None))
        starts = starts[: int(nk.value)]
        deo = np.searchsorted(starts, doc_offsets, side="left").astype(np.uint64)
        return starts, out[: int(nb.value) if text else 0], oo[: int(nk.value) + 1], deo

    def excerpts_batch_device(self, corpus, doc_offsets, starts=None, out_offsets=None, out=None, *, before, after=None,
                              sep=None, cap=None, cap_bytes=None, stream=None):
        """Device-resident excerpts on torch CUDA tensors: uint8 corpus (any alignment), int64/uint64 doc offsets, starts
        int64/uint64 [cap] or None, out_offsets int64/uint64 [cap + 1] or None, out uint8 [cap_bytes] (any alignment) or None
        (no bytes are copied).  -> (R, n_out_bytes, n_hits); raises AhaError(AHA_E_CAPACITY) when a buffer is too small
        (e.n_required = the excerpts, e.bytes_required = the bytes needed); nothing is written then."""
        import torch

        p, _alive = self._excerpt_params(before, after, sep)
        assert corpus.is_cuda and corpus.dtype == torch.uint8 and corpus.is_contiguous()
        assert doc_offsets.is_cuda and doc_offsets.dtype in (torch.int64, torch.uint64)
        for name, t in (("starts", starts), ("out_offsets", out_offsets)):
            if t is not None and not (t.is_cuda and t.dtype in (torch.int64, torch.uint64) and t.is_contiguous()):
                raise ValueError(name + " must be a contiguous int64/uint64 CUDA tensor")
        room = []
        if starts is not None:
            room.append(starts.numel())
        if out_offsets is not None:
            if out_offsets.numel() < 1:
                raise ValueError("out_offsets must have at least one entry")
            room.append(out_offsets.numel() - 1)
        cap = 0 if not room else min(room) if cap is None else min([int(cap)] + room)
        if out is not None:
            if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.dim() == 1):
                raise ValueError("out must be a contiguous one-dimensional uint8 CUDA tensor")
            cap_bytes = out.numel() if cap_bytes is None else min(int(cap_bytes), out.numel())
        else:
            cap_bytes = 0
        D = doc_offsets.numel() - 1
        nk, nb, nh = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        s = stream if stream is not None else torch.cuda.current_stream(corpus.device).cuda_stream
        rc = N.lib().aha_ac_grep_batch_device(
            self._h, corpus.data_ptr(), doc_offsets.data_ptr(), D, corpus.numel(), p, N.AHA_GREP_CONTEXT,
            starts.data_ptr() if starts is not None else None,
            out_offsets.data_ptr() if out_offsets is not None else None, cap,
            out.data_ptr() if out is not None else None, cap_bytes, C.byref(nk), C.byref(nb), C.byref(nh), C.c_void_p(s))
        if rc == N.AHA_E_CAPACITY:
            raise self._grep_capacity_error(rc, nk, nb)
        self._check(rc)
        return int(nk.value), int(nb.value), int(nh.value)

    def excerpts_corpus(self, corpus, before, after=None, sep=None, text=True):
        """excerpts_batch of a batch that already lives in HBM (DeviceCorpus), downloaded:
        -> (starts uint64[R], uint8 array, out_offsets uint64[R+1], n_hits)."""
        p, _alive = self._excerpt_params(before, after, sep)
        D, dev = corpus.n_docs, corpus.device
        nk, nb, nh = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        L = N.lib()
        flags = N.AHA_GREP_CONTEXT
        self._check(L.aha_ac_grep_batch_device(self._h, corpus.ptr, corpus.doc_ptr, D, corpus.n_bytes, p, flags, None, None,
                                               0, None, 0, C.byref(nk), C.byref(nb), C.byref(nh), None))
        cap, cap_bytes = int(nk.value), int(nb.value) if text else 0
        st, oo = DeviceBuffer(dev, max(cap, 1) * 8), DeviceBuffer(dev, (cap + 1) * 8)
        out = DeviceBuffer(dev, max(cap_bytes, 1)) if text else None
        self._check(L.aha_ac_grep_batch_device(self._h, corpus.ptr, corpus.doc_ptr, D, corpus.n_bytes, p, flags, st.ptr,
                                               oo.ptr, cap, out.ptr if text else None, cap_bytes, C.byref(nk), C.byref(nb),
                                               C.byref(nh), None))
        got = out.download(np.zeros(max(cap_bytes, 1), dtype=np.uint8))[:cap_bytes] if text else np.zeros(0, dtype=np.uint8)
        return (st.download(np.zeros(max(cap, 1), dtype=np.uint64))[:cap], got,
                oo.download(np.zeros(cap + 1, dtype=np.uint64)), int(nh.value))

    def excerpts(self, seq, before, after=None, sep=None):
        """The hits of match(seq, sep) in their context, as a list of (start, text).  bytes in: start is a byte offset and
        text is bytes.  str in: start is a character offset and text is a str (the contexts stay byte counts; no excerpt
        begins or ends inside a character)."""
        b = _b(seq)
        corpus = np.frombuffer(b, dtype=np.uint8)
        starts, out, oo, _ = self.excerpts_batch(corpus, np.array([0, len(b)], dtype=np.uint64), before, after, sep=sep)
        raw = out.tobytes()
        parts = [raw[int(oo[i]):int(oo[i + 1])] for i in range(starts.size)]
        if not isinstance(seq, str):
            return [(int(s), x) for s, x in zip(starts, parts)]
        lead = np.concatenate([[0], np.cumsum((corpus & 0xC0) != 0x80)])  # the characters that start in front of a byte
        return [(int(lead[int(s)]), x.decode("utf-8")) for s, x in zip(starts, parts)]

    # -- cover: which bytes lie inside a hit, and a redacted copy (aha_ac_cover_batch*) ---------------
    def _cover_host(self, corpus, doc_offsets, sep, want_mask, want_redacted, fill):
        if isinstance(corpus, (bytes, bytearray)):
            corpus = np.frombuffer(bytes(corpus), dtype=np.uint8)
        corpus = np.ascontiguousarray(corpus, dtype=np.uint8)
        doc_offsets = np.ascontiguousarray(doc_offsets, dtype=np.uint64)
        D = doc_offsets.size - 1
        n_bytes = int(doc_offsets[-1]) if doc_offsets.size else 0
        p = _params(False, sep)
        mask = np.zeros((n_bytes + 31) // 32, dtype=np.uint32) if want_mask else None
        red = np.zeros(n_bytes, dtype=np.uint8) if want_redacted else None
        cov = np.zeros(max(D, 0), dtype=np.uint64)
        nc, nh = C.c_uint64(0), C.c_uint64(0)
        rc = N.lib().aha_ac_cover_batch(self._h, _ptr(corpus), _ptr(doc_offsets), D, C.byref(p), 0, _ptr(mask), _ptr(red),
                                        int(fill) & 0xFF, _ptr(cov), C.byref(nc), C.byref(nh))
        self._check(rc)
        return mask, red, cov

    def cover_batch(self, corpus, doc_offsets, sep=None):
        """Which bytes of the batch lie inside a hit of match_batch(corpus, doc_offsets, sep), without the hit list:
        -> (mask uint32[ceil(N / 32)], doc_covered uint64[D]).  Bit j of the batch is word j >> 5, bit j & 31
        (np.unpackbits(mask.view(np.uint8), bitorder="little")[:N]); doc_covered[d] = covered bytes of document d."""
        mask, _, cov = self._cover_host(corpus, doc_offsets, sep, True, False, 0)
        return mask, cov

    def redact_batch(self, corpus, doc_offsets, fill=0x2A, sep=None):
        """The batch with every byte inside a hit replaced by `fill`: -> (redacted uint8[N], doc_covered uint64[D])."""
        _, red, cov = self._cover_host(corpus, doc_offsets, sep, False, True, fill)
        return red, cov

    def cover(self, seq, sep=None):
        """np.bool_[n_bytes]: True where the byte of `seq` (bytes, or str as UTF-8) lies inside a hit of match(seq, sep)."""
        b = _b(seq)
        mask, _ = self.cover_batch(np.frombuffer(b, dtype=np.uint8), np.array([0, len(b)], dtype=np.uint64), sep=sep)
        return np.unpackbits(mask.view(np.uint8), bitorder="little")[: len(b)].astype(np.bool_)

    def redact(self, seq, fill="*", sep=None):
        """`seq` with what the keys cover blanked out.  bytes in, bytes out: every covered byte becomes `fill` (a byte, an int
        or a one-character str).  str in, str out: every character that has a covered byte becomes `fill` (a str)."""
        if isinstance(seq, str):
            b = seq.encode("utf-8")
            cov = self.cover(b, sep=sep)
            raw = np.frombuffer(b, dtype=np.uint8)
            lead = (raw & 0xC0) != 0x80  # a character starts here
            hit = np.zeros(int(lead.sum()), dtype=np.int64)
            np.add.at(hit, np.cumsum(lead) - 1, cov)
            f = fill if isinstance(fill, str) else bytes([int(fill) & 0xFF]).decode("latin-1")
            return "".join(f if h else ch for ch, h in zip(seq, hit))
        f = fill
        if isinstance(f, str):
            f = f.encode("utf-8")
        if isinstance(f, (bytes, bytearray)):
            if len(f) != 1:
                raise ValueError("fill must be one byte for a bytes sequence")
            f = f[0]
        b = _b(seq)
        red, _ = self.redact_batch(np.frombuffer(b, dtype=np.uint8), np.array([0, len(b)], dtype=np.uint64), fill=f, sep=sep)
        return red.tobytes()

    def cover_batch_device(self, corpus, doc_offsets, mask=None, redacted=None, fill=0x2A, doc_covered=None, sep=None,
                           stream=None):
        """Device-resident cover on torch CUDA tensors: uint8 corpus, int64/uint64 doc offsets; mask int32/uint32
        [ceil(N / 32)] or None; redacted uint8 [N] or None (the corpus tensor itself: redaction in place); doc_covered
        int64/uint64 [D] or None.  -> (n_covered, n_hits)."""
        import torch

        assert corpus.is_cuda and corpus.dtype == torch.uint8 and corpus.is_contiguous()
        assert doc_offsets.is_cuda and doc_offsets.dtype in (torch.int64, torch.uint64)
        n_bytes, D = corpus.numel(), doc_offsets.numel() - 1
        if mask is not None and not (mask.is_cuda and mask.dtype in (torch.int32, torch.uint32) and mask.is_contiguous()
                                     and mask.numel() >= (n_bytes + 31) // 32):
            raise ValueError("mask must be a contiguous int32/uint32 CUDA tensor of at least ceil(N / 32) entries")
        if redacted is not None and not (redacted.is_cuda and redacted.dtype == torch.uint8 and redacted.is_contiguous()
                                         and redacted.numel() >= n_bytes):
            raise ValueError("redacted must be a contiguous uint8 CUDA tensor of at least N entries")
        if doc_covered is not None and not (doc_covered.is_cuda and doc_covered.dtype in (torch.int64, torch.uint64)
                                            and doc_covered.is_contiguous() and doc_covered.numel() >= D):
            raise ValueError("doc_covered must be a contiguous int64/uint64 CUDA tensor of at least D entries")
        p = _params(False, sep)
        nc, nh = C.c_uint64(0), C.c_uint64(0)
        s = stream if stream is not None else torch.cuda.current_stream(corpus.device).cuda_stream
        rc = N.lib().aha_ac_cover_batch_device(
            self._h, corpus.data_ptr(), doc_offsets.data_ptr(), D, n_bytes, C.byref(p), 0,
            mask.data_ptr() if mask is not None else None, redacted.data_ptr() if redacted is not None else None,
            int(fill) & 0xFF, doc_covered.data_ptr() if doc_covered is not None else None, C.byref(nc), C.byref(nh), C.c_void_p(s))
        self._check(rc)
        return int(nc.value), int(nh.value)

    def cover_corpus(self, corpus, sep=None, redacted=False, fill=0x2A):
        """Cover of a batch that already lives in HBM (DeviceCorpus), downloaded:
        -> (mask uint32[ceil(N / 32)], redacted uint8[N] or None, doc_covered uint64[D], n_covered, n_hits).  The corpus on the
        device stays as it is (the redacted copy goes to a buffer of its own)."""
        D, n_bytes = corpus.n_docs, corpus.n_bytes
        n_words = (n_bytes + 31) // 32
        p = _params(False, sep)
        dev = corpus.device
        d_mask = DeviceBuffer(dev, max(n_words, 1) * 4)
        d_cov = DeviceBuffer(dev, max(D, 1) * 8)
        d_red = DeviceBuffer(dev, max(n_bytes, 1)) if redacted else None
        nc, nh = C.c_uint64(0), C.c_uint64(0)
        rc = N.lib().aha_ac_cover_batch_device(self._h, corpus.ptr, corpus.doc_ptr, D, n_bytes, C.byref(p), 0, d_mask.ptr,
                                               d_red.ptr if d_red else None, int(fill) & 0xFF, d_cov.ptr, C.byref(nc),
                                               C.byref(nh), None)
        self._check(rc)
        mask = d_mask.download(np.zeros(n_words, dtype=np.uint32))
        red = d_red.download(np.zeros(n_bytes, dtype=np.uint8)) if d_red else None
        return mask, red, d_cov.download(np.zeros(D, dtype=np.uint64)), int(nc.value), int(nh.value)

    # -- exchange format of the multi-GPU all-gatherv: {end, value} pairs <-> Hit triples ------------
    def hits_pack_device(self, hits, n, pairs, stream=None):
        """hits [>=n,3] int32 -> pairs [>=n,2] int32, both on the handle's device (asynchronous)."""
        import torch

        assert hits.is_cuda and pairs.is_cuda and hits.dtype == pairs.dtype == torch.int32
        assert hits.is_contiguous() and pairs.is_contiguous() and hits.numel() >= 3 * n and pairs.numel() >= 2 * n
        s = stream if stream is not None else torch.cuda.current_stream(hits.device).cuda_stream
        self._check(N.lib().aha_ac_hits_pack_device(self._h, hits.data_ptr(), n, pairs.data_ptr(), C.c_void_p(s)))

    def hits_unpack_device(self, pairs, n, hits, chars=False, stream=None):
        """pairs [>=n,2] int32 -> hits [>=n,3] int32 (start = end - key length), asynchronous."""
        import torch

        assert hits.is_cuda and pairs.is_cuda and hits.dtype == pairs.dtype == torch.int32
        assert hits.is_contiguous() and pairs.is_contiguous() and hits.numel() >= 3 * n and pairs.numel() >= 2 * n
        s = stream if stream is not None else torch.cuda.current_stream(hits.device).cuda_stream
        self._check(N.lib().aha_ac_hits_unpack_device(self._h, pairs.data_ptr(), n, 1 if chars else 0,
                                                      hits.data_ptr(), C.c_void_p(s)))

    def stream_format(self):
        """(step_bits, len_bits) of the 4-byte exchange stream's words for this automaton (include/aha_hip.h)."""
        sb, lb = C.c_uint32(0), C.c_uint32(0)
        self._check(N.lib().aha_ac_stream_format(self._h, C.byref(sb), C.byref(lb)))
        return int(sb.value), int(lb.value)

    def hits_pack4_device(self, hits, n, words, n_words, stream=None):
        """hits [>=n,3] int32 -> the 4-byte exchange stream in `words` (int32, capacity >= 2n + ceil(n/1024)); the
        stream length lands in n_words[0] (int64 device tensor).  Asynchronous."""
        import torch

        assert hits.is_cuda and words.is_cuda and n_words.is_cuda and hits.dtype == words.dtype == torch.int32
        assert n_words.dtype == torch.int64 and hits.is_contiguous() and words.is_contiguous() and hits.numel() >= 3 * n
        s = stream if stream is not None else torch.cuda.current_stream(hits.device).cuda_stream
        self._check(N.lib().aha_ac_hits_pack4_device(self._h, hits.data_ptr(), n, words.data_ptr(), words.numel(),
                                                     n_words.data_ptr(), C.c_void_p(s)))

    def hits_unpack4_device(self, words, n, hits, chars=False, stream=None):
        """4-byte exchange stream of n hits -> hits [>=n,3] int32, asynchronous."""
        import torch

        assert hits.is_cuda and words.is_cuda and hits.dtype == words.dtype == torch.int32
        assert hits.is_contiguous() and words.is_contiguous() and hits.numel() >= 3 * n
        s = stream if stream is not None else torch.cuda.current_stream(hits.device).cuda_stream
        self._check(N.lib().aha_ac_hits_unpack4_device(self._h, words.data_ptr(), n, 1 if chars else 0,
                                                       hits.data_ptr(), C.c_void_p(s)))

    def hits_unpack4_segs_device(self, words, segs, hits, chars=False, stream=None):
        """Several 4-byte streams inside `words` -> their places in `hits`, ONE launch: segs = [(word offset of the
        stream, its hit count, row offset in hits), ...] (at most 64)."""
        import torch

        assert hits.is_cuda and words.is_cuda and hits.dtype == words.dtype == torch.int32
        assert hits.is_contiguous() and words.is_contiguous()
        arr = (N.aha_stream_seg * max(len(segs), 1))()
        for k, (wo, n, oo) in enumerate(segs):
            assert hits.numel() >= 3 * (oo + n)
            arr[k].word_offset, arr[k].n_hits, arr[k].out_offset = int(wo), int(n), int(oo)
        s = stream if stream is not None else torch.cuda.current_stream(hits.device).cuda_stream
        self._check(N.lib().aha_ac_hits_unpack4_segs_device(self._h, words.data_ptr(), arr, len(segs),
                                                            1 if chars else 0, hits.data_ptr(), C.c_void_p(s)))

    @property
    def n_keys(self):
        return self.info["n_keys"]

    def key_lengths(self, chars=False):
        """Length of every key in bytes (or in chars): Hit#end - Hit#start of its hits."""
        ln = self.export(N.AHA_IMG_KEY_LN, np.uint32).reshape(-1, 2)[:, 0].astype(np.int32)
        if chars:
            return self.export(N.AHA_IMG_KEY_KC, np.uint32).astype(np.int32) + 1
        return ln

    def export(self, which, dtype):
        """One array of the automaton image (data; host-logic tests, debugging)."""
        n = N.lib().aha_ac_export(self._h, which, None, 0)
        if n < 0:
            raise AhaError(int(n))
        buf = np.zeros(int(n) // np.dtype(dtype).itemsize, dtype=dtype)
        if n:
            N.lib().aha_ac_export(self._h, which, _ptr(buf), int(n))
        return buf

    # -- feeds: sequences that arrive in pieces (aha_feed_*) -----------------------------------------
    def feed(self, n_seqs, chars=False, sep=None, longest=0, fold=False):
        """n_seqs open sequences matched piece by piece (aha_feed_open): see Feed.  chars: offsets and bases in characters.
        sep: a BitArray -- the feed's match and count calls apply the separator filter of match(seq, sep) to the whole sequence
        (aha_feed_open_params): a hit is reported one byte late, and Feed.finish ends a sequence.
        longest: 1 or 2 -- a longest feed: its match calls report what match_longest(seq, intersectable = False | True) of the
        whole sequence yields, each hit in the call that holds the byte at which it is yielded, and Feed.finish reports the hit
        that is still pending and ends the sequence.  Refused (AHA_E_INVALID): longest with sep or chars, and count, cover,
        select, replace and grep calls on such a feed.
        fold: on a handle compiled with fold_simple, fold_bmp or fold_kana a FOLDED feed (AHA_FEED_FOLD; without it such a handle
        has no feeds: the library's AHA_E_INVALID is raised): every call answers as if the sequence ended with its piece -- a
        character cut between two calls is folded whole, one still open at a call's end is matched unfolded, so for keys that
        are whole characters the hits are those of the whole sequence folded as one document.  match, count and cover calls
        (redactor included: the original bytes outside hits); select, replace and grep calls, sep and longest are refused.  On any
        other handle fold changes nothing."""
        h = C.c_void_p()
        flags = (N.AHA_FEED_CHARS if chars else 0) | (N.AHA_FEED_FOLD if fold else 0)
        if sep is None and not longest:
            rc = N.lib().aha_feed_open(self._h, int(n_seqs), flags, C.byref(h))
        else:
            p = _params(False, sep, longest)
            rc = N.lib().aha_feed_open_params(self._h, int(n_seqs), flags, C.byref(p), C.byref(h))
        self._check(rc)
        return Feed(self, h, int(n_seqs), chars, sep, int(longest))

    def set_profiling(self, enabled=True):
        self._check(N.lib().aha_ac_set_profiling(self._h, 1 if enabled else 0))

    def release_scratch(self):
        """Frees the handle's grow-only device scratch."""
        self._check(N.lib().aha_ac_release_scratch(self._h))

    def scratch_bytes(self):
        """Device bytes the handle currently holds as scratch (all scratch sets)."""
        return int(N.lib().aha_ac_scratch_bytes(self._h))

    def last_timing(self):
        t = N.aha_timing()
        t.struct_size = C.sizeof(t)
        self._check(N.lib().aha_ac_last_timing(self._h, C.byref(t)))
        return {f: getattr(t, f) for f, _ in t._fields_ if f != "struct_size"}


class Feed:
    """Sequences that arrive in pieces across calls (aha_feed_*).  Each call matches a batch of pieces -- piece d is the next
    part of sequence seq_ids[d] -- and yields exactly the hits one plain match over the whole sequence so far would report with
    an end inside the piece; a count call (count_batch, count) gives the same hits per key, a cover call (cover_batch,
    redact_batch, cover, redact, redactor) the bytes they cover.  Offsets are relative to the piece (start may be negative: the hit began in an earlier piece);
    piece_bases[d] is the sequence's length before it, so base + offset is absolute.  A feed opened with sep (AC.feed(..,
    sep=BitArray)) filters match and count calls as match(seq, sep) of the whole sequence does: a call reports the surviving
    hits that end before the piece's last byte -- one that ended with the piece before has end == 0 -- and finish_batch /
    finish report those that end with the sequence and start it again; cover, select, replace and grep calls are refused
    there.  A grep call (grep_batch, grepper) gives the lines that close in the call and have a hit.
    A longest feed (AC.feed(.., longest=1 | 2); Feed.longest) is match_longest in pieces: a call that takes a sequence from n0
    to n1 bytes reports the hits of match_longest(whole sequence) that are yielded at a byte in [n0, n1) -- a hit may lie
    wholly in earlier pieces (start >= -Lmax, end >= -(Lmax - 1)) -- and finish_batch / finish report the one hit still
    pending and start the sequence again; count, cover, select, replace and grep calls are refused there."""

    def __init__(self, ac, handle, n_seqs, chars, sep=None, longest=0):
        self._ac, self._h, self.n_seqs, self.chars, self.sep, self.longest = ac, handle, n_seqs, chars, sep, longest

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                N.lib().aha_feed_free(h)
            except Exception:  # interpreter shutdown
                pass

    __del__ = close

    def _check(self, rc):
        if self._h is None:
            raise AhaError(N.AHA_E_INVALID, "feed is closed")
        self._ac._check(rc)

    def reset(self, seq=None):
        """Sequence seq (None: every sequence) starts again from length 0."""
        self._check(N.lib().aha_feed_reset(self._h, 0xFFFFFFFF if seq is None else int(seq)))

    def position(self, seq):
        """(bytes, chars) fed to sequence seq so far (chars counted on char feeds only)."""
        b, c = C.c_uint64(0), C.c_uint64(0)
        self._check(N.lib().aha_feed_position(self._h, int(seq), C.byref(b), C.byref(c)))
        return int(b.value), int(c.value)

    # -- what the batch methods share: the pieces of a host or a device call, optional device outputs, the capacity error ------
    @staticmethod
    def _pieces_host(corpus, piece_offsets, seq_ids):
        """-> (corpus uint8, piece_offsets uint64, seq_ids uint32, D): contiguous arrays; corpus may come as bytes."""
        if isinstance(corpus, (bytes, bytearray)):
            corpus = np.frombuffer(bytes(corpus), dtype=np.uint8)
        corpus = np.ascontiguousarray(corpus, dtype=np.uint8)
        piece_offsets = np.ascontiguousarray(piece_offsets, dtype=np.uint64)
        seq_ids = np.ascontiguousarray(seq_ids, dtype=np.uint32)
        D = piece_offsets.size - 1
        if seq_ids.size != D:
            raise ValueError("one sequence id per piece")
        return corpus, piece_offsets, seq_ids, D

    @staticmethod
    def _pieces_device(corpus, piece_offsets, seq_ids, stream):
        """-> (D, n_bytes, the stream's handle): stream None is torch's current stream on the corpus' device."""
        import torch

        assert corpus.is_cuda and corpus.dtype == torch.uint8 and corpus.is_contiguous()
        assert piece_offsets.is_cuda and piece_offsets.dtype in (torch.int64, torch.uint64) and piece_offsets.is_contiguous()
        assert seq_ids.is_cuda and seq_ids.dtype in (torch.int32, torch.uint32) and seq_ids.is_contiguous()
        D = piece_offsets.numel() - 1
        assert seq_ids.numel() >= D
        return D, corpus.numel(), stream if stream is not None else torch.cuda.current_stream(corpus.device).cuda_stream

    @staticmethod
    def _opt64(*pairs):
        """(tensor, n) pairs: each tensor None or a contiguous int64/uint64 CUDA tensor of at least n entries."""
        import torch

        for t, n in pairs:
            assert t is None or (t.is_cuda and t.dtype in (torch.int64, torch.uint64) and t.is_contiguous() and t.numel() >= n)

    @staticmethod
    def _opt32(*pairs):
        """... or a contiguous int32/uint32 one."""
        import torch

        for t, n in pairs:
            assert t is None or (t.is_cuda and t.dtype in (torch.int32, torch.uint32) and t.is_contiguous() and t.numel() >= n)

    @staticmethod
    def _capacity(rc, n, attr):
        """The AhaError of a call that did not fit; what is needed goes into .required or .n_required, as each method documents."""
        e = AhaError(rc)
        setattr(e, attr, int(n.value))
        return e

    def match_batch(self, corpus, piece_offsets, seq_ids, cap=None):
        """Host buffers: -> (hits, piece_hit_offsets uint64[D+1], piece_bases uint64[D])."""
        corpus, piece_offsets, seq_ids, D = self._pieces_host(corpus, piece_offsets, seq_ids)
        pho = np.zeros(D + 1, dtype=np.uint64)
        bases = np.zeros(max(D, 1), dtype=np.uint64)
        if cap is None:
            cap = max(64, corpus.size // 8)
        while True:
            out = np.zeros(max(cap, 1), dtype=HIT_DTYPE)
            n = C.c_uint64(0)
            rc = N.lib().aha_feed_match_batch(self._h, _ptr(corpus), _ptr(piece_offsets), _ptr(seq_ids), D, _ptr(out), cap,
                                              _ptr(pho), _ptr(bases), C.byref(n))
            if rc == N.AHA_E_CAPACITY:
                cap = int(n.value)
                continue
            self._check(rc)
            return out[: n.value], pho, bases[:D]

    def match_batch_device(self, corpus, piece_offsets, seq_ids, out, piece_hit_offsets=None, piece_bases=None, stream=None):
        """Device-resident form on torch CUDA tensors (uint8 corpus, int64/uint64 piece offsets, int32/uint32 sequence ids,
        int32 [cap, 3] out, int64/uint64 [D+1] / [D] or None).  Returns the hit count; raises AhaError(AHA_E_CAPACITY) with
        .required when out is too small (the feed is then unchanged)."""
        import torch

        D, n_bytes, s = self._pieces_device(corpus, piece_offsets, seq_ids, stream)
        assert out.is_cuda and out.dtype == torch.int32 and out.is_contiguous()
        self._opt64((piece_hit_offsets, D + 1), (piece_bases, D))
        n = C.c_uint64(0)
        rc = N.lib().aha_feed_match_batch_device(
            self._h, corpus.data_ptr(), piece_offsets.data_ptr(), seq_ids.data_ptr(), D, n_bytes, out.data_ptr(), out.numel() // 3,
            _dptr(piece_hit_offsets), _dptr(piece_bases), C.byref(n), C.c_void_p(s))
        if rc == N.AHA_E_CAPACITY:
            raise self._capacity(rc, n, "required")
        self._check(rc)
        return int(n.value)

    # -- a feed with a separator filter or a longest feed: the named sequences end here (aha_feed_finish_batch*) ------
    def finish_batch(self, seq_ids, cap=None):
        """The surviving hits that end with the named sequences, relative to each sequence's end (end == 0, start == -len):
        -> (hits, seq_hit_offsets uint64[n+1], bases uint64[n] = the sequences' lengths).  The sequences start again at length
        0.  On a longest feed: the one hit of each sequence that is still pending (end <= 0).  Only on a feed opened with sep
        or longest."""
        seq_ids = np.ascontiguousarray(seq_ids, dtype=np.uint32)
        D = seq_ids.size
        sho = np.zeros(D + 1, dtype=np.uint64)
        bases = np.zeros(max(D, 1), dtype=np.uint64)
        if cap is None:
            cap = max(16, 4 * D)
        while True:
            out = np.zeros(max(cap, 1), dtype=HIT_DTYPE)
            n = C.c_uint64(0)
            rc = N.lib().aha_feed_finish_batch(self._h, _ptr(seq_ids), D, _ptr(out), cap, _ptr(sho), _ptr(bases), C.byref(n))
            if rc == N.AHA_E_CAPACITY:  # (the sequences have not restarted: the same call again)
                cap = int(n.value)
                continue
            self._check(rc)
            return out[: n.value], sho, bases[:D]

    def finish_batch_device(self, seq_ids, out, seq_hit_offsets=None, bases=None, stream=None):
        """Device-resident form on torch CUDA tensors (int32/uint32 sequence ids, int32 [cap, 3] out, int64/uint64 [n+1] / [n]
        or None).  Returns the hit count; raises AhaError(AHA_E_CAPACITY) with .required when out is too small (the sequences
        have then not restarted)."""
        import torch

        assert seq_ids.is_cuda and seq_ids.dtype in (torch.int32, torch.uint32) and seq_ids.is_contiguous()
        assert out.is_cuda and out.dtype == torch.int32 and out.is_contiguous()
        D = seq_ids.numel()
        self._opt64((seq_hit_offsets, D + 1), (bases, D))
        n = C.c_uint64(0)
        s = stream if stream is not None else torch.cuda.current_stream(out.device).cuda_stream
        rc = N.lib().aha_feed_finish_batch_device(self._h, seq_ids.data_ptr() if D else None, D, out.data_ptr(), out.numel() // 3,
                                                  _dptr(seq_hit_offsets), _dptr(bases), C.byref(n), C.c_void_p(s))
        if rc == N.AHA_E_CAPACITY:
            raise self._capacity(rc, n, "required")
        self._check(rc)
        return int(n.value)

    def finish(self, seq):
        """Sequence seq ends here: the surviving hits that end with it, as Hits with absolute offsets; it starts again."""
        hits, _, bases = self.finish_batch(np.array([seq], dtype=np.uint32))
        base = int(bases[0])
        return [Hit(int(h["start"]) + base, int(h["end"]) + base, int(h["value"])) for h in hits]

    def count_batch(self, corpus, piece_offsets, seq_ids, per_key=True, accumulate_into=None):
        """Hits per key of match_batch on the same pieces, without the hit list (aha_feed_count_batch): -> (key_counts
        uint64[K] or None, piece_hit_offsets uint64[D+1], piece_bases uint64[D]).  The sequences move on as a match call would
        move them.  accumulate_into: a uint64[K] array the counts are added to (AHA_COUNT_ACCUMULATE); it is also what is
        returned, and a call that fails leaves it as it was."""
        corpus, piece_offsets, seq_ids, D = self._pieces_host(corpus, piece_offsets, seq_ids)
        K = self._ac.n_keys
        flags = 0
        kc = None
        if accumulate_into is not None:
            kc = accumulate_into
            if not (isinstance(kc, np.ndarray) and kc.dtype == np.uint64 and kc.flags.c_contiguous and kc.flags.writeable
                    and kc.size == K):
                raise ValueError(f"accumulate_into must be a writeable C-contiguous uint64 array of {K} entries")
            flags = N.AHA_COUNT_ACCUMULATE
        elif per_key:
            kc = np.zeros(K, dtype=np.uint64)
        pho = np.zeros(D + 1, dtype=np.uint64)
        bases = np.zeros(max(D, 1), dtype=np.uint64)
        n = C.c_uint64(0)
        rc = N.lib().aha_feed_count_batch(self._h, _ptr(corpus), _ptr(piece_offsets), _ptr(seq_ids), D, flags, _ptr(kc),
                                          _ptr(pho), _ptr(bases), C.byref(n))
        self._check(rc)
        return kc, pho, bases[:D]

    def count_batch_device(self, corpus, piece_offsets, seq_ids, key_counts=None, piece_hit_offsets=None, piece_bases=None,
                           accumulate=False, stream=None):
        """Device-resident count on torch CUDA tensors (uint8 corpus, int64/uint64 piece offsets, int32/uint32 sequence ids;
        key_counts int64/uint64 [K] or None; int64/uint64 [D+1] / [D] or None).  Returns the hit count.  accumulate: add into
        key_counts."""
        import torch

        D, n_bytes, s = self._pieces_device(corpus, piece_offsets, seq_ids, stream)
        K = self._ac.n_keys
        if key_counts is not None and not (key_counts.is_cuda and key_counts.dtype in (torch.int64, torch.uint64)
                                           and key_counts.is_contiguous() and key_counts.numel() >= K):
            raise ValueError(f"key_counts must be a contiguous int64/uint64 CUDA tensor of at least {K} entries")
        self._opt64((piece_hit_offsets, D + 1), (piece_bases, D))
        n = C.c_uint64(0)
        rc = N.lib().aha_feed_count_batch_device(
            self._h, corpus.data_ptr(), piece_offsets.data_ptr(), seq_ids.data_ptr(), D, n_bytes,
            N.AHA_COUNT_ACCUMULATE if accumulate else 0, _dptr(key_counts), _dptr(piece_hit_offsets), _dptr(piece_bases),
            C.byref(n), C.c_void_p(s))
        self._check(rc)
        return int(n.value)

    def count(self, seq, piece):
        """The next piece of one sequence: the hits per key that match(seq, piece) would give, uint64[K]."""
        b = _b(piece)
        kc, _, _ = self.count_batch(np.frombuffer(b, dtype=np.uint8), np.array([0, len(b)], dtype=np.uint64),
                                    np.array([seq], dtype=np.uint32))
        return kc

    # -- feed cover: the mask and the redacted copy of pieces, straddling hits included (aha_feed_cover_batch*) ---------
    def _cover_host(self, corpus, piece_offsets, seq_ids, want_mask, want_redacted, fill):
        corpus, piece_offsets, seq_ids, D = self._pieces_host(corpus, piece_offsets, seq_ids)
        n_bytes = int(piece_offsets[-1])
        mask = np.zeros((n_bytes + 31) // 32, dtype=np.uint32) if want_mask else None
        red = np.zeros(n_bytes, dtype=np.uint8) if want_redacted else None
        back = np.zeros(max(D, 1), dtype=np.uint32)
        cov = np.zeros(max(D, 1), dtype=np.uint64)
        pho = np.zeros(D + 1, dtype=np.uint64)
        bases = np.zeros(max(D, 1), dtype=np.uint64)
        nc, nh = C.c_uint64(0), C.c_uint64(0)
        rc = N.lib().aha_feed_cover_batch(self._h, _ptr(corpus), _ptr(piece_offsets), _ptr(seq_ids), D, 0, _ptr(mask), _ptr(red),
                                          _fill_byte(fill), _ptr(back), _ptr(cov), _ptr(pho), _ptr(bases), C.byref(nc),
                                          C.byref(nh))
        self._check(rc)
        return mask, red, {"piece_back": back[:D], "piece_covered": cov[:D], "piece_hit_offsets": pho, "piece_bases": bases[:D],
                           "n_covered": int(nc.value), "n_hits": int(nh.value)}

    def cover_batch(self, corpus, piece_offsets, seq_ids):
        """Which bytes of the pieces lie inside a hit of their sequences, without the hit list (aha_feed_cover_batch):
        -> (mask uint32[ceil(N / 32)], info) in the layout of AC.cover_batch.  info: piece_back uint32[D] (the bytes in front
        of the piece that lie inside a hit ending in it: they belong to earlier pieces), piece_covered uint64[D],
        piece_hit_offsets uint64[D + 1], piece_bases uint64[D], n_covered, n_hits.  The sequences move on as a match call
        would move them."""
        mask, _, info = self._cover_host(corpus, piece_offsets, seq_ids, True, False, 0)
        return mask, info

    def redact_batch(self, corpus, piece_offsets, seq_ids, fill=0x2A):
        """The pieces with every byte inside a hit replaced by `fill`: -> (redacted uint8[N], info as for cover_batch).  The
        last info["piece_back"][d] bytes of the sequence in front of piece d are covered as well."""
        _, red, info = self._cover_host(corpus, piece_offsets, seq_ids, False, True, fill)
        return red, info

    def cover_batch_device(self, corpus, piece_offsets, seq_ids, mask=None, redacted=None, fill=0x2A, piece_back=None,
                           piece_covered=None, piece_hit_offsets=None, piece_bases=None, stream=None):
        """Device-resident feed cover on torch CUDA tensors: uint8 corpus, int64/uint64 piece offsets, int32/uint32 sequence
        ids; mask int32/uint32 [ceil(N / 32)] or None; redacted uint8 [N] or None (the corpus tensor itself: in place);
        piece_back int32/uint32 [D], piece_covered and piece_bases int64/uint64 [D], piece_hit_offsets [D + 1], each or None.
        -> (n_covered, n_hits)."""
        import torch

        D, n_bytes, s = self._pieces_device(corpus, piece_offsets, seq_ids, stream)
        if mask is not None and not (mask.is_cuda and mask.dtype in (torch.int32, torch.uint32) and mask.is_contiguous()
                                     and mask.numel() >= (n_bytes + 31) // 32):
            raise ValueError("mask must be a contiguous int32/uint32 CUDA tensor of at least ceil(N / 32) entries")
        if redacted is not None and not (redacted.is_cuda and redacted.dtype == torch.uint8 and redacted.is_contiguous()
                                         and redacted.numel() >= n_bytes):
            raise ValueError("redacted must be a contiguous uint8 CUDA tensor of at least N entries")
        if piece_back is not None and not (piece_back.is_cuda and piece_back.dtype in (torch.int32, torch.uint32)
                                           and piece_back.is_contiguous() and piece_back.numel() >= D):
            raise ValueError("piece_back must be a contiguous int32/uint32 CUDA tensor of at least D entries")
        self._opt64((piece_covered, D), (piece_hit_offsets, D + 1), (piece_bases, D))
        nc, nh = C.c_uint64(0), C.c_uint64(0)
        rc = N.lib().aha_feed_cover_batch_device(
            self._h, corpus.data_ptr(), piece_offsets.data_ptr(), seq_ids.data_ptr(), D, n_bytes, 0, _dptr(mask), _dptr(redacted),
            _fill_byte(fill), _dptr(piece_back), _dptr(piece_covered), _dptr(piece_hit_offsets), _dptr(piece_bases), C.byref(nc),
            C.byref(nh), C.c_void_p(s))
        self._check(rc)
        return int(nc.value), int(nh.value)

    def cover(self, seq, piece):
        """The next piece of one sequence: -> (np.bool_[len(piece)], back).  True where the byte lies inside a hit of the
        sequence; the `back` bytes in front of the piece lie inside a hit that ends in it."""
        b = _b(piece)
        mask, info = self.cover_batch(np.frombuffer(b, dtype=np.uint8), np.array([0, len(b)], dtype=np.uint64),
                                      np.array([seq], dtype=np.uint32))
        return np.unpackbits(mask.view(np.uint8), bitorder="little")[: len(b)].astype(np.bool_), int(info["piece_back"][0])

    def redact(self, seq, piece, fill="*"):
        """The next piece of one sequence with what the keys cover blanked out: -> (bytes, back).  The last `back` bytes
        handed out before for this sequence are covered too (Feed.redactor keeps them back until they are final)."""
        b = _b(piece)
        red, info = self.redact_batch(np.frombuffer(b, dtype=np.uint8), np.array([0, len(b)], dtype=np.uint64),
                                      np.array([seq], dtype=np.uint32), fill=fill)
        return red.tobytes(), int(info["piece_back"][0])

    def redactor(self, fill="*"):
        """A Redactor over this feed: push(seq, piece) / finish(seq) give the redacted stream of every sequence."""
        return Redactor(self, fill)

    # -- feed select: leftmost-longest, non-overlapping hits of sequences in pieces (aha_feed_select_batch*) ------------
    def select_batch(self, corpus, piece_offsets, seq_ids, final=False, cap=None):
        """The selected hits that this call settles (aha_feed_select_batch): for piece d, which takes its sequence from n0 to
        n1 bytes, the hits of select(sequence so far) with a start in [F(n0), F(n1)), F(n) = max(0, n - (Lmax - 1)) -- up to
        n1 with final=True, after which the named sequences start again from length 0.  -> (hits HIT_DTYPE, info) with
        offsets relative to the piece (start may be negative, end may be <= 0) and info = {"piece_sel_offsets" uint64[D+1],
        "piece_bases" uint64[D], "piece_hold" uint32[D]: the bytes at the end of the sequence whose fate is still open,
        "n_hits"}.  Byte feeds only, and only for sequences fed through select calls alone since their last reset.
        cap None: a sizing call first (a call that does not fit changes nothing)."""
        return self._select_host(corpus, piece_offsets, seq_ids, N.AHA_FEED_SELECT_FINAL if final else 0, cap, "piece_sel_offsets")

    def _select_host(self, corpus, piece_offsets, seq_ids, flags, cap, key):
        """aha_feed_select_batch with `flags`; key: the info name of the pieces' offsets into the result"""
        corpus, piece_offsets, seq_ids, D = self._pieces_host(corpus, piece_offsets, seq_ids)
        pso = np.zeros(D + 1, dtype=np.uint64)
        bases = np.zeros(max(D, 1), dtype=np.uint64)
        hold = np.zeros(max(D, 1), dtype=np.uint32)
        n, nh = C.c_uint64(0), C.c_uint64(0)
        L = N.lib()
        if cap is None:
            rc = L.aha_feed_select_batch(self._h, _ptr(corpus), _ptr(piece_offsets), _ptr(seq_ids), D, flags, None, 0, _ptr(pso),
                                         _ptr(bases), _ptr(hold), C.byref(n), C.byref(nh))
            if rc != N.AHA_E_CAPACITY:
                self._check(rc)
                return np.zeros(0, dtype=HIT_DTYPE), {key: pso, "piece_bases": bases[:D], "piece_hold": hold[:D],
                                                      "n_hits": int(nh.value)}
            cap = int(n.value)
        out = np.zeros(max(int(cap), 1), dtype=HIT_DTYPE)
        rc = L.aha_feed_select_batch(self._h, _ptr(corpus), _ptr(piece_offsets), _ptr(seq_ids), D, flags, _ptr(out), int(cap),
                                     _ptr(pso), _ptr(bases), _ptr(hold), C.byref(n), C.byref(nh))
        if rc == N.AHA_E_CAPACITY:
            raise self._capacity(rc, n, "n_required")
        self._check(rc)
        return out[: int(n.value)], {key: pso, "piece_bases": bases[:D], "piece_hold": hold[:D], "n_hits": int(nh.value)}

    def select_batch_device(self, corpus, piece_offsets, seq_ids, out, piece_sel_offsets=None, piece_bases=None,
                            piece_hold=None, final=False, cap=None, stream=None, _flags=0):
        """Device-resident form on torch CUDA tensors: uint8 corpus, int64/uint64 piece offsets, int32/uint32 sequence ids,
        out int32 [cap, 3] or None (a sizing call), piece_sel_offsets / piece_bases int64/uint64 [D+1] / [D] or None,
        piece_hold int32/uint32 [D] or None.  -> (n_selected, n_hits); raises AhaError(AHA_E_CAPACITY) when out is too small
        (e.n_required = the hits needed); nothing is written then and the feed is unchanged."""
        import torch

        D, n_bytes, s = self._pieces_device(corpus, piece_offsets, seq_ids, stream)
        if out is not None:
            if not (out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and out.dim() == 2 and out.shape[1] == 3):
                raise ValueError("out must be a contiguous int32 CUDA tensor of shape [cap, 3]")
            cap = out.shape[0] if cap is None else min(int(cap), out.shape[0])
        else:
            cap = 0
        self._opt64((piece_sel_offsets, D + 1), (piece_bases, D))
        self._opt32((piece_hold, D))
        n, nh = C.c_uint64(0), C.c_uint64(0)
        rc = N.lib().aha_feed_select_batch_device(
            self._h, corpus.data_ptr(), piece_offsets.data_ptr(), seq_ids.data_ptr(), D, n_bytes,
            (N.AHA_FEED_SELECT_FINAL if final else 0) | _flags, _dptr(out) if cap else None, cap, _dptr(piece_sel_offsets),
            _dptr(piece_bases),
            _dptr(piece_hold), C.byref(n), C.byref(nh), C.c_void_p(s))
        if rc == N.AHA_E_CAPACITY:
            raise self._capacity(rc, n, "n_required")
        self._check(rc)
        return int(n.value), int(nh.value)

    def select(self, seq, piece, final=False):
        """The next piece of one sequence: the selected hits it settles, as Hits with absolute offsets, ascending by start."""
        b = _b(piece)
        hits, info = self.select_batch(np.frombuffer(b, dtype=np.uint8), np.array([0, len(b)], dtype=np.uint64),
                                       np.array([seq], dtype=np.uint32), final=final)
        base = int(info["piece_bases"][0])
        return [Hit(s + base, e + base, v) for s, e, v in hits.tolist()]

    # -- feed tokens: dictionary segmentation of sequences in pieces (aha_feed_select_batch* with AHA_FEED_SELECT_TOKENS) ---
    @staticmethod
    def _token_flags(final, gap_runs):
        return (N.AHA_FEED_SELECT_FINAL if final else 0) | N.AHA_FEED_SELECT_TOKENS | (N.AHA_FEED_SELECT_GAP_RUNS if gap_runs else 0)

    def tokens_batch(self, corpus, piece_offsets, seq_ids, final=False, gap_runs=False, cap=None):
        """The tokens that this call settles (aha_feed_select_batch with AHA_FEED_SELECT_TOKENS): per sequence the feed keeps a
        token cursor t behind which everything has been reported; the call reports the tokens of the sequence from t up to
        the select cursor it leaves, without the last where nothing yet says that it ends there (a character whose next lead
        byte has not arrived).  With gap_runs gaps are not cut into characters and are handed out in parts as they come;
        with final=True everything is reported and the named sequences start again from length 0.  -> (tokens HIT_DTYPE, info)
        with offsets relative to the piece, value = the key or -1, and info = {"piece_tok_offsets" uint64[D+1], "piece_bases"
        uint64[D], "piece_hold" uint32[D]: the bytes behind t, "n_hits"}.  The tokens of a sequence's calls, made absolute
        and concatenated, are AC.tokens_batch of the whole (with gap_runs: after joining -1 tokens that touch).  Byte feeds
        only, and only for sequences fed through token calls alone since their last reset or final call.  cap None: a sizing
        call first (a call that does not fit changes nothing)."""
        return self._select_host(corpus, piece_offsets, seq_ids, self._token_flags(final, gap_runs), cap, "piece_tok_offsets")

    def tokens_batch_device(self, corpus, piece_offsets, seq_ids, out, piece_tok_offsets=None, piece_bases=None, piece_hold=None,
                            final=False, gap_runs=False, cap=None, stream=None):
        """Device-resident form on torch CUDA tensors, as select_batch_device: out int32 [cap, 3] or None (a sizing call).
        -> (n_tokens, n_hits); raises AhaError(AHA_E_CAPACITY) when out is too small (e.n_required = the tokens needed); nothing
        is written then and the feed is unchanged."""
        return self.select_batch_device(corpus, piece_offsets, seq_ids, out, piece_tok_offsets, piece_bases, piece_hold, final=final,
                                        cap=cap, stream=stream, _flags=self._token_flags(False, gap_runs))

    def tokens(self, seq, piece, final=False, gap_runs=False):
        """The next piece of one sequence: the tokens it settles, as Hits with absolute offsets (value -1: no key)."""
        b = _b(piece)
        toks, info = self.tokens_batch(np.frombuffer(b, dtype=np.uint8), np.array([0, len(b)], dtype=np.uint64),
                                       np.array([seq], dtype=np.uint32), final=final, gap_runs=gap_runs)
        base = int(info["piece_bases"][0])
        return [Hit(s + base, e + base, v) for s, e, v in toks.tolist()]

    def segmenter(self, gap_runs=False):
        """A Segmenter over this feed: push(seq, piece) / finish(seq) give the tokens of every sequence with their bytes."""
        return Segmenter(self, gap_runs)

    # -- feed replace: the substituted stream of sequences in pieces, built on the device (aha_feed_replace_batch*) --------
    def replace_batch(self, corpus, piece_offsets, seq_ids, repl_or_table, final=False):
        """Every piece's share of the substituted stream (aha_feed_replace_batch): for piece d, which takes its sequence from
        n0 to n1 bytes and moves its select cursor from c0 to c1, the bytes T[c0..c1) with every hit the call settles
        (select_batch of the same pieces) replaced as the table says -- a ReplTable of the feed's handle, or what
        AC.replacements takes.  With final=True everything settles and the named sequences start again from length 0.
        -> (uint8 array, info) with info = {"piece_out_offsets" uint64[D+1], "piece_bases" uint64[D], "piece_hold" uint32[D],
        "n_selected", "n_hits"}; piece d's bytes are out[piece_out_offsets[d]:piece_out_offsets[d+1]], and the pieces'
        bytes of one sequence, concatenated, are AC.replace of the whole.  A sizing call first (it changes nothing)."""
        corpus, piece_offsets, seq_ids, D = self._pieces_host(corpus, piece_offsets, seq_ids)
        table = self._ac._table(repl_or_table)
        flags = N.AHA_FEED_REPLACE_FINAL if final else 0
        poo = np.zeros(D + 1, dtype=np.uint64)
        bases = np.zeros(max(D, 1), dtype=np.uint64)
        hold = np.zeros(max(D, 1), dtype=np.uint32)
        n, ns, nh = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        L = N.lib()
        rc = L.aha_feed_replace_batch(self._h, table._h, _ptr(corpus), _ptr(piece_offsets), _ptr(seq_ids), D, flags, None, 0,
                                      _ptr(poo), _ptr(bases), _ptr(hold), C.byref(n), C.byref(ns), C.byref(nh))
        out = np.zeros(0, dtype=np.uint8)
        if rc == N.AHA_E_CAPACITY:
            cap = int(n.value)
            out = np.zeros(cap, dtype=np.uint8)
            rc = L.aha_feed_replace_batch(self._h, table._h, _ptr(corpus), _ptr(piece_offsets), _ptr(seq_ids), D, flags,
                                          _ptr(out), cap, _ptr(poo), _ptr(bases), _ptr(hold), C.byref(n), C.byref(ns),
                                          C.byref(nh))
        self._check(rc)
        return out[: int(n.value)], {"piece_out_offsets": poo, "piece_bases": bases[:D], "piece_hold": hold[:D],
                                     "n_selected": int(ns.value), "n_hits": int(nh.value)}

    def replace_batch_device(self, corpus, piece_offsets, seq_ids, table, out, piece_out_offsets=None, piece_bases=None,
                             piece_hold=None, final=False, cap=None, stream=None):
        """Device-resident form on torch CUDA tensors: uint8 corpus, int64/uint64 piece offsets, int32/uint32 sequence ids, a
        ReplTable, out uint8 [cap] (any alignment) or None (a sizing call), piece_out_offsets / piece_bases int64/uint64
        [D+1] / [D] or None, piece_hold int32/uint32 [D] or None.  -> (n_out_bytes, n_selected, n_hits); raises
        AhaError(AHA_E_CAPACITY) when out is too small (e.n_required = the bytes needed); nothing is written then and the
        feed is unchanged."""
        import torch

        D, n_bytes, s = self._pieces_device(corpus, piece_offsets, seq_ids, stream)
        if out is not None:
            if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.dim() == 1):
                raise ValueError("out must be a contiguous one-dimensional uint8 CUDA tensor")
            cap = out.numel() if cap is None else min(int(cap), out.numel())
        else:
            cap = 0
        self._opt64((piece_out_offsets, D + 1), (piece_bases, D))
        self._opt32((piece_hold, D))
        n, ns, nh = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        rc = N.lib().aha_feed_replace_batch_device(
            self._h, table._h, corpus.data_ptr(), piece_offsets.data_ptr(), seq_ids.data_ptr(), D, n_bytes,
            N.AHA_FEED_REPLACE_FINAL if final else 0, _dptr(out) if cap else None, cap, _dptr(piece_out_offsets),
            _dptr(piece_bases), _dptr(piece_hold), C.byref(n), C.byref(ns), C.byref(nh), C.c_void_p(s))
        if rc == N.AHA_E_CAPACITY:
            raise self._capacity(rc, n, "n_required")
        self._check(rc)
        return int(n.value), int(ns.value), int(nh.value)

    def replace(self, seq, piece, repl_or_table, final=False):
        """The next piece of one sequence: the substituted bytes that can no longer change (bytes); with final=True the rest,
        and the sequence starts again from length 0.  b"".join of a sequence's results == matcher.replace(whole, repl)."""
        b = _b(piece)
        out, _ = self.replace_batch(np.frombuffer(b, dtype=np.uint8), np.array([0, len(b)], dtype=np.uint64),
                                    np.array([seq], dtype=np.uint32), repl_or_table, final=final)
        return out.tobytes()

    def replacer(self, repl):
        """A Replacer over this feed: push(seq, piece) / finish(seq) give the substituted stream of every sequence."""
        return Replacer(self, repl)

    # -- feed grep: the lines of sequences in pieces that have a hit (aha_feed_grep_batch*) ------------------------------------
    def grep_batch(self, corpus, piece_offsets, seq_ids, delim=b"\n", invert=False, final=False, text=True):
        """The fragments of this call's pieces that close in it and are kept (aha_feed_grep_batch).  The pieces are split
        as AC.records(corpus, piece_offsets, delim) splits them; a fragment closes when it ends with the delimiter, or under
        final=True; it is kept when (its record, matched as its own document, has a hit) != invert -- a piece's first
        fragment may continue a record that earlier pieces left open.  -> (kept_recs uint64[n_kept], uint8 array,
        rec_out_offsets uint64[n_kept+1], info) with info = {"piece_rec_offsets", "piece_kept_offsets" uint64[D+1],
        "piece_hold" uint32[D]: the bytes at the end of the piece that belong to the record left open -- the caller keeps them,
        "piece_head" uint64[D]: the held bytes to emit in front of the piece's first kept fragment, "piece_bases",
        "piece_rec_bases" uint64[D], "n_recs", "n_hits"}.  With final=True the named sequences start again from length 0.
        Byte feeds only, one delimiter per feed, and only for sequences fed through grep calls alone since their last reset.
        text False: no bytes are copied.  A sizing call first (a call that does not fit changes nothing)."""
        corpus, piece_offsets, seq_ids, D = self._pieces_host(corpus, piece_offsets, seq_ids)
        d = _delim_byte(delim)
        flags = (N.AHA_GREP_INVERT if invert else 0) | (N.AHA_FEED_GREP_FINAL if final else 0)
        pro, pko = np.zeros(D + 1, dtype=np.uint64), np.zeros(D + 1, dtype=np.uint64)
        hold = np.zeros(max(D, 1), dtype=np.uint32)
        head, bases, rbases = (np.zeros(max(D, 1), dtype=np.uint64) for _ in range(3))
        nr, nk, nb, nh = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        L = N.lib()

        def call(kept, roo, cap_recs, out, cap_bytes):
            return L.aha_feed_grep_batch(self._h, _ptr(corpus), _ptr(piece_offsets), _ptr(seq_ids), D, d, flags, _ptr(kept),
                                         _ptr(roo), cap_recs, _ptr(out) if text else None, cap_bytes, _ptr(pro), _ptr(pko),
                                         _ptr(hold), _ptr(head), _ptr(bases), _ptr(rbases), C.byref(nr), C.byref(nk),
                                         C.byref(nb), C.byref(nh))

        # (a buffer with no room: the call succeeds only where nothing is kept)
        kept, roo, out = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint8)
        rc = call(kept, roo, 0, out, 0)
        if rc == N.AHA_E_CAPACITY:
            cap_recs, cap_bytes = int(nk.value), int(nb.value) if text else 0
            kept, roo = np.zeros(max(cap_recs, 1), dtype=np.uint64), np.zeros(cap_recs + 1, dtype=np.uint64)
            out = np.zeros(max(cap_bytes, 1), dtype=np.uint8)
            rc = call(kept, roo, cap_recs, out, cap_bytes)
        self._check(rc)
        n = int(nk.value)
        info = {"piece_rec_offsets": pro, "piece_kept_offsets": pko, "piece_hold": hold[:D], "piece_head": head[:D],
                "piece_bases": bases[:D], "piece_rec_bases": rbases[:D], "n_recs": int(nr.value), "n_hits": int(nh.value)}
        return kept[:n], out[: int(nb.value) if text else 0], roo[: n + 1], info

    def grep_batch_device(self, corpus, piece_offsets, seq_ids, kept_recs=None, rec_out_offsets=None, out=None, delim=b"\n",
                          invert=False, final=False, piece_rec_offsets=None, piece_kept_offsets=None, piece_hold=None,
                          piece_head=None, piece_bases=None, piece_rec_bases=None, cap_recs=None, cap_bytes=None, stream=None):
        """Device-resident form on torch CUDA tensors: uint8 corpus (any alignment), int64/uint64 piece offsets, int32/uint32
        sequence ids, kept_recs int64/uint64 [cap_recs] or None, rec_out_offsets int64/uint64 [cap_recs + 1] or None, out
        uint8 [cap_bytes] or None (no bytes are copied), the per-piece outputs int64/uint64 [D+1] / [D] (piece_hold
        int32/uint32 [D]) or None.  -> (n_recs, n_kept, n_out_bytes, n_hits); raises AhaError(AHA_E_CAPACITY) when a buffer is
        too small (e.n_required = the fragments needed, e.bytes_required = the bytes needed); nothing is written then and the
        feed is unchanged."""
        import torch

        D, n_bytes, s = self._pieces_device(corpus, piece_offsets, seq_ids, stream)
        for name, t in (("kept_recs", kept_recs), ("rec_out_offsets", rec_out_offsets)):
            if t is not None and not (t.is_cuda and t.dtype in (torch.int64, torch.uint64) and t.is_contiguous()):
                raise ValueError(name + " must be a contiguous int64/uint64 CUDA tensor")
        room = []
        if kept_recs is not None:
            room.append(kept_recs.numel())
        if rec_out_offsets is not None:
            if rec_out_offsets.numel() < 1:
                raise ValueError("rec_out_offsets must have at least one entry")
            room.append(rec_out_offsets.numel() - 1)
        cap_recs = 0 if not room else min(room) if cap_recs is None else min([int(cap_recs)] + room)
        if out is not None:
            if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.dim() == 1):
                raise ValueError("out must be a contiguous one-dimensional uint8 CUDA tensor")
            cap_bytes = out.numel() if cap_bytes is None else min(int(cap_bytes), out.numel())
        else:
            cap_bytes = 0
        self._opt64((piece_rec_offsets, D + 1), (piece_kept_offsets, D + 1), (piece_head, D), (piece_bases, D),
                    (piece_rec_bases, D))
        self._opt32((piece_hold, D))
        nr, nk, nb, nh = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        rc = N.lib().aha_feed_grep_batch_device(
            self._h, corpus.data_ptr(), piece_offsets.data_ptr(), seq_ids.data_ptr(), D, n_bytes, _delim_byte(delim),
            (N.AHA_GREP_INVERT if invert else 0) | (N.AHA_FEED_GREP_FINAL if final else 0), _dptr(kept_recs),
            _dptr(rec_out_offsets), cap_recs, _dptr(out), cap_bytes, _dptr(piece_rec_offsets), _dptr(piece_kept_offsets),
            _dptr(piece_hold), _dptr(piece_head), _dptr(piece_bases), _dptr(piece_rec_bases), C.byref(nr), C.byref(nk),
            C.byref(nb), C.byref(nh), C.c_void_p(s))
        if rc == N.AHA_E_CAPACITY:
            raise AC._grep_capacity_error(rc, nk, nb)
        self._check(rc)
        return int(nr.value), int(nk.value), int(nb.value), int(nh.value)

    def grepper(self, delim=b"\n", invert=False):
        """A Grepper over this feed: push(seq, piece) / finish(seq) give the kept lines of every sequence."""
        return Grepper(self, delim, invert)

    def match(self, seq, piece):
        """The next piece of one sequence: its hits as Hits with absolute offsets."""
        b = _b(piece)
        hits, _, bases = self.match_batch(np.frombuffer(b, dtype=np.uint8), np.array([0, len(b)], dtype=np.uint64),
                                          np.array([seq], dtype=np.uint32))
        base = int(bases[0])
        return [Hit(int(h["start"]) + base, int(h["end"]) + base, int(h["value"])) for h in hits]


class Redactor:
    """Redaction of sequences that arrive in pieces (Feed.redactor).  A hit that straddles a cut covers up to W = Lmax - 1
    bytes of what came before, so the last min(W, length) redacted bytes of every sequence are held on the host:
    push(seq, piece) returns only bytes that can no longer change, finish(seq) the rest, and
    b"".join(pushes) + finish(seq) == matcher.redact(whole sequence)."""

    def __init__(self, feed, fill="*"):
        self._feed, self._fill = feed, _fill_byte(fill)
        self._W = max(int(feed._ac.info["max_key_len"]) - 1, 0)
        self._held = {}

    def push(self, seq, piece):
        red, back = self._feed.redact(seq, piece, fill=self._fill)
        held = bytearray(self._held.get(seq, b""))
        if back:
            held[len(held) - back:] = bytes([self._fill]) * back
        held += red
        keep = min(self._W, len(held))
        self._held[seq] = bytes(held[len(held) - keep:])
        return bytes(held[: len(held) - keep])

    def finish(self, seq):
        """The bytes still held for seq; the sequence starts again from length 0."""
        out = self._held.pop(seq, b"")
        self._feed.reset(seq)
        return out


class Replacer:
    """Substitution in sequences that arrive in pieces (Feed.replacer), host arithmetic on Feed.select_batch.  repl means what
    it means for AC.replace: a mapping from key index to replacement (a key it does not name, or that maps to None, is kept)
    or a sequence with one entry per key; "" deletes.  push(seq, piece) returns the substituted bytes that can no longer
    change, finish(seq) the rest, and b"".join(pushes) + finish(seq) == matcher.replace(whole sequence, repl) as bytes.  Per
    sequence at most W = Lmax - 1 source bytes are held on the host: those behind the cursor (piece_hold)."""

    def __init__(self, feed, repl):
        self._feed, self._repl = feed, repl
        self._n_keys = feed._ac.n_keys
        self._held = {}  # seq -> the source bytes behind the cursor

    def _step(self, seq, piece, final):
        b = _b(piece)
        hits, info = self._feed.select_batch(np.frombuffer(b, dtype=np.uint8), np.array([0, len(b)], dtype=np.uint64),
                                             np.array([seq], dtype=np.uint32), final=final)
        # held || piece = the sequence from the old cursor on; the piece's first byte is at len(held) of it
        held = self._held.get(seq, b"")
        src = held + b
        hold = int(info["piece_hold"][0])
        done = len(src) - hold
        if hits.size:
            hits = hits.copy()
            hits["start"] += len(held)
            hits["end"] += len(held)
        out = substitute(src[:done], hits, self._repl, self._n_keys)
        if hold:
            self._held[seq] = src[done:]
        else:
            self._held.pop(seq, None)
        return out

    def push(self, seq, piece):
        return self._step(seq, piece, False)

    def finish(self, seq):
        """The bytes still open for seq, substituted; the sequence starts again from length 0."""
        return self._step(seq, b"", True)


class Segmenter:
    """Dictionary segmentation of sequences that arrive in pieces (Feed.segmenter), host arithmetic on Feed.tokens_batch.
    push(seq, piece) returns the tokens that can no longer change as [(token bytes, key or -1)], finish(seq) the rest, and
    b"".join of all token bytes is the sequence.  In character mode the tokens are those of AC.segment of the whole sequence;
    with gap_runs the parts of a gap are handed out as they come.  The bytes behind the token cursor (piece_hold) are held on
    the host: a character that arrives byte by byte has no length limit, the feed's state per sequence has."""

    def __init__(self, feed, gap_runs=False):
        self._feed, self._gap_runs = feed, bool(gap_runs)
        self._held = {}  # seq -> the source bytes behind the token cursor

    def _step(self, seq, piece, final):
        b = _b(piece)
        toks, info = self._feed.tokens_batch(np.frombuffer(b, dtype=np.uint8), np.array([0, len(b)], dtype=np.uint64),
                                             np.array([seq], dtype=np.uint32), final=final, gap_runs=self._gap_runs)
        # held || piece = the sequence from the old token cursor on; the piece's first byte is at len(held) of it
        held = self._held.get(seq, b"")
        src = held + b
        hold = int(info["piece_hold"][0])
        out = [(src[s + len(held):e + len(held)], v) for s, e, v in toks.tolist()]
        if hold:
            self._held[seq] = src[len(src) - hold:]
        else:
            self._held.pop(seq, None)
        return out

    def push(self, seq, piece):
        return self._step(seq, piece, False)

    def finish(self, seq):
        """The tokens still open for seq; the sequence starts again from length 0."""
        return self._step(seq, b"", True)


class Grepper:
    """Grep over sequences that arrive in pieces whose ends fall in the middle of lines (Feed.grepper), host arithmetic on
    Feed.grep_batch.  push(seq, piece) returns the kept lines that closed with this piece -- each with its delimiter, as
    bytes --, finish(seq) the trailing line without one if it is kept, and pushes + finish(seq), concatenated, are
    matcher.grep(whole sequence, delim, invert) as bytes.  The bytes of the line that is still open are held on the host
    (piece_hold): a line has no length limit, the feed's state per sequence has."""

    def __init__(self, feed, delim=b"\n", invert=False):
        self._feed, self._delim, self._invert = feed, _delim_byte(delim), bool(invert)
        self._held = {}  # seq -> the bytes of the open line

    def _step(self, seq, piece, final):
        b = _b(piece)
        _, out, roo, info = self._feed.grep_batch(np.frombuffer(b, dtype=np.uint8), np.array([0, len(b)], dtype=np.uint64),
                                                  np.array([seq], dtype=np.uint32), delim=self._delim, invert=self._invert,
                                                  final=final)
        raw = out.tobytes()
        lines = [raw[int(roo[i]):int(roo[i + 1])] for i in range(roo.size - 1)]
        held = self._held.get(seq, b"")
        head, hold = int(info["piece_head"][0]), int(info["piece_hold"][0])
        if head:  # the open line closed and is kept: it stands in front of the piece's first kept fragment
            if lines:
                lines[0] = held[len(held) - head:] + lines[0]
            else:  # (an empty piece under final: the line closes without a fragment)
                lines = [held[len(held) - head:]]
        if final:
            held = b""
        elif hold == len(b):
            held = held + b
        else:
            held = b[len(b) - hold:]
        if held:
            self._held[seq] = held
        else:
            self._held.pop(seq, None)
        return lines

    def push(self, seq, piece):
        return self._step(seq, piece, False)

    def finish(self, seq):
        """The open line of seq if it is kept; the sequence starts again from length 0."""
        return self._step(seq, b"", True)


# Aha::ACBig = ACX(Int64) (src/aha/ac.cr:9): node ids of 64 bits, the same Hit with an Int32 value (ac.cr:273) -- the
# library's numbering has no such limit below 2^31 keys, so one class answers for both names.
ACBig = AC


class DeviceBuffer:
    """HBM obtained through the C ABI (aha_buffer_alloc): what a caller without a GPU framework uses."""

    def __init__(self, device, n_bytes):
        self.device, self.n_bytes = device, int(n_bytes)
        p = C.c_void_p()
        rc = N.lib().aha_buffer_alloc(device, self.n_bytes, C.byref(p))
        if rc != N.AHA_OK:
            raise AhaError(rc, N.lib().aha_last_error(None).decode() or None)
        self.ptr = p

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.n_bytes
        rc = N.lib().aha_buffer_upload(self.device, self.ptr, _ptr(arr), arr.nbytes)
        if rc != N.AHA_OK:
            raise AhaError(rc, N.lib().aha_last_error(None).decode() or None)

    def download(self, arr):
        assert arr.flags["C_CONTIGUOUS"] and arr.nbytes <= self.n_bytes
        rc = N.lib().aha_buffer_download(self.device, _ptr(arr), self.ptr, arr.nbytes)
        if rc != N.AHA_OK:
            raise AhaError(rc, N.lib().aha_last_error(None).decode() or None)
        return arr

    def __del__(self):
        p, self.ptr = getattr(self, "ptr", None), None
        if p:
            try:
                N.lib().aha_buffer_free(self.device, p)
            except Exception:  # interpreter shutdown
                pass


class DeviceCorpus:
    """A batch resident in HBM (aha_corpus_upload): bytes of all documents + D + 1 offsets, validated on upload."""

    def __init__(self, corpus, doc_offsets, device=0):
        if isinstance(corpus, (bytes, bytearray)):
            corpus = np.frombuffer(bytes(corpus), dtype=np.uint8)
        corpus = np.ascontiguousarray(corpus, dtype=np.uint8)
        doc_offsets = np.ascontiguousarray(doc_offsets, dtype=np.uint64)
        h = C.c_void_p()
        rc = N.lib().aha_corpus_upload(device, _ptr(corpus), _ptr(doc_offsets), doc_offsets.size - 1, C.byref(h))
        if rc != N.AHA_OK:
            raise AhaError(rc, N.lib().aha_last_error(None).decode() or None)
        self._h = h
        self.device = device
        self.n_docs = int(N.lib().aha_corpus_n_docs(h))
        self.n_bytes = int(N.lib().aha_corpus_n_bytes(h))
        self.ptr = C.c_void_p(N.lib().aha_corpus_bytes(h))
        self.doc_ptr = C.c_void_p(N.lib().aha_corpus_doc_offsets(h))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                N.lib().aha_corpus_free(h)
            except Exception:  # interpreter shutdown
                pass


class ACGroup:
    """Several GPUs of one node behind one object (aha_group_*, include/aha_hip.h): contiguous byte-balanced
    document ranges, one per device entry, all-gatherv of the hit buffers (RCCL between distinct devices)."""

    def __init__(self, handle):
        self._h = handle

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                N.lib().aha_group_free(h)
            except Exception:  # interpreter shutdown
                pass

    @classmethod
    def compile(cls, keys, devices, host_only=False, fold_ascii=False):
        blob, offs = _pack_keys(keys)
        return cls.compile_packed(blob, offs, devices, host_only, fold_ascii)

    @classmethod
    def compile_packed(cls, blob, offs, devices, host_only=False, fold_ascii=False):
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        dev = np.ascontiguousarray(devices, dtype=np.int32)
        h = C.c_void_p()
        ek = C.c_uint32(0)
        rc = N.lib().aha_group_compile(_ptr(blob), _ptr(offs), offs.size - 1, _ptr(dev), dev.size,
                                       (N.AHA_OPT_HOST_ONLY if host_only else 0) | (N.AHA_OPT_FOLD_ASCII if fold_ascii else 0),
                                       C.byref(h), C.byref(ek))
        if rc != N.AHA_OK:
            raise AhaError(rc, key_index=ek.value)
        return cls(h)

    @staticmethod
    def partition(doc_offsets, n_parts):
        doc_offsets = np.ascontiguousarray(doc_offsets, dtype=np.uint64)
        bounds = np.zeros(n_parts + 1, dtype=np.uint64)
        rc = N.lib().aha_group_partition(_ptr(doc_offsets), doc_offsets.size - 1, n_parts, _ptr(bounds))
        if rc != N.AHA_OK:
            raise AhaError(rc)
        return bounds

    def match_batch(self, corpus, doc_offsets, chars=False, cap=None, longest=0):
        """AC.match_batch over the group's shards (longest: as there)."""
        if isinstance(corpus, (bytes, bytearray)):
            corpus = np.frombuffer(bytes(corpus), dtype=np.uint8)
        corpus = np.ascontiguousarray(corpus, dtype=np.uint8)
        doc_offsets = np.ascontiguousarray(doc_offsets, dtype=np.uint64)
        D = doc_offsets.size - 1
        p = _params(chars, None, longest)
        dho = np.zeros(D + 1, dtype=np.uint64)
        if cap is None:
            cap = max(64, corpus.size // 8)
        while True:
            out = np.zeros(cap, dtype=HIT_DTYPE)
            n = C.c_uint64(0)
            rc = N.lib().aha_group_match_batch(self._h, _ptr(corpus), _ptr(doc_offsets), D, C.byref(p), _ptr(out), cap,
                                               _ptr(dho), C.byref(n))
            if rc == N.AHA_E_CAPACITY:
                cap = int(n.value)
                continue
            if rc != N.AHA_OK:
                raise AhaError(rc, N.lib().aha_group_last_error(self._h).decode() or None)
            return out[: n.value], dho

    def upload_corpus(self, corpus, doc_offsets):
        """The batch resident on the group's devices (aha_group_corpus_upload): every shard's document range on its device."""
        if isinstance(corpus, (bytes, bytearray)):
            corpus = np.frombuffer(bytes(corpus), dtype=np.uint8)
        corpus = np.ascontiguousarray(corpus, dtype=np.uint8)
        doc_offsets = np.ascontiguousarray(doc_offsets, dtype=np.uint64)
        h = C.c_void_p()
        rc = N.lib().aha_group_corpus_upload(self._h, _ptr(corpus), _ptr(doc_offsets), doc_offsets.size - 1, C.byref(h))
        if rc != N.AHA_OK:
            raise AhaError(rc, N.lib().aha_group_last_error(self._h).decode() or None)
        return GroupCorpus(self, h, doc_offsets.size - 1)

    def match_corpus(self, gcorpus, chars=False):
        """aha_group_match_batch_device: every device matches its resident range, then the all-gatherv; the hits stay on the
        devices (download_shard reads one device's copy of the whole stream).  Returns (n_hits, per-document offsets)."""
        p = _params(chars, None)
        dho = np.zeros(gcorpus.n_docs + 1, dtype=np.uint64)
        n = C.c_uint64(0)
        rc = N.lib().aha_group_match_batch_device(self._h, gcorpus._h, C.byref(p), _ptr(dho), C.byref(n))
        if rc != N.AHA_OK:
            raise AhaError(rc, N.lib().aha_group_last_error(self._h).decode() or None)
        return int(n.value), dho

    def download_shard(self, shard):
        """The gathered hit stream as device `shard` holds it after the last match_batch (every device holds it all)."""
        n = C.c_uint64(0)
        N.lib().aha_group_download_shard(self._h, shard, None, 0, C.byref(n))
        out = np.zeros(max(int(n.value), 1), dtype=HIT_DTYPE)
        rc = N.lib().aha_group_download_shard(self._h, shard, _ptr(out), out.size, C.byref(n))
        if rc != N.AHA_OK:
            raise AhaError(rc, N.lib().aha_group_last_error(self._h).decode() or None)
        return out[: n.value]

    def last_timing(self):
        t = N.aha_group_timing()
        rc = N.lib().aha_group_last_timing(self._h, C.byref(t))
        if rc != N.AHA_OK:
            raise AhaError(rc)
        return {f: getattr(t, f) for f, _ in t._fields_ if f != "struct_size"}


class GroupCorpus:
    """A batch resident on the devices of an ACGroup (aha_group_corpus_*); keeps its group alive."""

    def __init__(self, group, handle, n_docs):
        self._g, self._h, self.n_docs = group, handle, n_docs

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                N.lib().aha_group_corpus_free(h)
            except Exception:  # interpreter shutdown
                pass
