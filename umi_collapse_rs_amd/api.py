"""Host-side mirror of the reference's plugin interface for the hot path, on top
of the C ABI (include/umihip.h):

    trait DataStruct  (src/data/mod.rs:11-17)   -> HipNaive
    trait Algorithm   (src/algo/mod.rs:13-20)    -> Directional, Adjacency, Cluster
    bucket loop       (src/deduplicate_sam.rs:207-233) -> Context.dedup_batch

Same names, argument meaning and error behaviour as the reference (where the
reference panics, these raise).  Everything computes on the GPU through
libumihip.so; there is no CPU path in this package."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (UMI_ALGO_ADJACENCY, UMI_ALGO_CLUSTER, UMI_ALGO_DIRECTIONAL, UMI_CELLS_CR22, Stats, UmiHipError, check, load, ptr)


def to_bitset(umis, umi_len=None):
    """utils::to_bitset (src/utils/mod.rs:63-83) for a batch: list of str/bytes or a
    uint8 array [n*umi_len] -> (keys u64[n], nmask u64[n])."""
    if isinstance(umis, np.ndarray):
        raw = np.ascontiguousarray(umis, dtype=np.uint8)
        assert umi_len, "umi_len is required for a raw byte array"
        n = raw.size // umi_len
    else:
        bs = [u.encode() if isinstance(u, str) else bytes(u) for u in umis]
        n = len(bs)
        umi_len = umi_len or (len(bs[0]) if bs else 1)
        if any(len(b) != umi_len for b in bs):
            raise ValueError("all UMIs of a run have the same length (umi_length)")
        raw = np.frombuffer(b"".join(bs), dtype=np.uint8)
    keys = np.zeros(n, dtype=np.uint64)
    nmask = np.zeros(n, dtype=np.uint64)
    check(load().umi_encode_umis(ptr(raw, C.c_uint8), n, umi_len, ptr(keys, C.c_uint64),
                                 ptr(nmask, C.c_uint64)))
    return keys, nmask


def to_bitset_wide(umis, umi_len):
    """to_bitset (src/utils/mod.rs:63-83) for UMIs of any length up to 85: (keys, nmask) uint64 [n, n_words]."""
    w = (3 * umi_len + 63) // 64
    buf = np.frombuffer("".join(umis).encode(), dtype=np.uint8)
    keys = np.zeros((len(umis), w), dtype=np.uint64)
    nm = np.zeros((len(umis), w), dtype=np.uint64)
    check(load().umi_encode_umis_wide(ptr(buf, C.c_uint8), len(umis), umi_len, w, ptr(keys, C.c_uint64),
                                      ptr(nm, C.c_uint64)))
    return keys, nm


def to_bitset_seq(seqs, n_words=None):
    """to_bitset (src/utils/mod.rs:63-83) per read for whole reads of up to 256 bases and of any
    lengths: list of str/bytes -> (keys, nmask) uint64 [n, n_words], n_words = ceil(3 * longest / 64)
    unless given; the words behind a read's own are zero (umi_encode_seqs)."""
    bs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    off = np.zeros(len(bs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
    if n_words is None:
        n_words = max(1, (3 * max([len(b) for b in bs] or [0]) + 63) // 64)
    buf = np.frombuffer(b"".join(bs) or b"\0", dtype=np.uint8)
    keys = np.zeros((len(bs), n_words), dtype=np.uint64)
    nm = np.zeros((len(bs), n_words), dtype=np.uint64)
    check(load().umi_encode_seqs(ptr(buf, C.c_uint8), ptr(off, C.c_uint64), len(bs), n_words,
                                 ptr(keys, C.c_uint64), ptr(nm, C.c_uint64)))
    return keys, nm


def partition_buckets(bucket_off, n_ranks):
    """umi_partition_buckets: owner rank of every bucket (uint32[n_buckets]), the assignment the
    multi-device context uses -- for hosts that run one process per GPU."""
    bucket_off = np.ascontiguousarray(bucket_off, dtype=np.uint64)
    nb = max(0, len(bucket_off) - 1)
    owner = np.zeros(nb, dtype=np.uint32)
    check(load().umi_partition_buckets(ptr(bucket_off, C.c_uint64), nb, n_ranks, ptr(owner, C.c_uint32)))
    return owner


class Context:
    """One GPU context (umi_ctx): one per process in a one-process-per-GPU job; or, with a list
    of device ids, one context over several GPUs of the node (umi_ctx_create_multi: dedup_batch
    shards its buckets over them)."""

    def __init__(self, device_id=0, profile=False):
        self._h = C.c_void_p()
        if isinstance(device_id, (list, tuple)):
            ids = (C.c_int * len(device_id))(*[int(d) for d in device_id])
            check(load().umi_ctx_create_multi(ids, len(device_id), C.byref(self._h)))
        else:
            check(load().umi_ctx_create(device_id, C.byref(self._h)))
        self.device_id = device_id
        if profile:
            self.set_option("profile", 1)

    def set_option(self, name, value):
        check(load().umi_ctx_set_option(self._h, name.encode(), int(value)))

    def counter(self, name):
        """what the context has done since it was created (umi_ctx_get_counter)"""
        v = C.c_uint64(0)
        check(load().umi_ctx_get_counter(self._h, name.encode(), C.byref(v)))
        return int(v.value)

    def close(self):
        if getattr(self, "_h", None):
            load().umi_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def dedup_batch(self, keys, nmask, freq, bucket_off, umi_len, k=1, percentage=0.5,
                    algo=UMI_ALGO_DIRECTIONAL, adj_max_freq=0, want_root=True):
        """Host-buffer batched call.  Returns (kept u8[N], root u32[N] or None, stats dict)."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        freq = np.ascontiguousarray(freq, dtype=np.int32)
        bucket_off = np.ascontiguousarray(bucket_off, dtype=np.uint64)
        nm = None if nmask is None else np.ascontiguousarray(nmask, dtype=np.uint64)
        n = len(keys)
        if len(freq) != n or (nm is not None and len(nm) != n):
            raise ValueError("keys/nmask/freq lengths differ")
        if len(bucket_off) < 1 or (len(bucket_off) > 1 and int(bucket_off[-1]) != n):
            raise ValueError("bucket_off[-1] must equal len(keys)")
        kept = np.zeros(n, dtype=np.uint8)
        root = np.zeros(n, dtype=np.uint32) if want_root else None
        st = Stats()
        check(load().umi_dedup_batch(self._h, ptr(keys, C.c_uint64), ptr(nm, C.c_uint64),
                                     ptr(freq, C.c_int32), ptr(bucket_off, C.c_uint64),
                                     len(bucket_off) - 1, umi_len, k, percentage, algo,
                                     adj_max_freq, ptr(kept, C.c_uint8), ptr(root, C.c_uint32),
                                     C.byref(st)))
        return kept, root, st.as_dict()

    def dedup_batch_edit(self, keys, nmask, freq, bucket_off, umi_len, k=1, percentage=0.5,
                         algo=UMI_ALGO_DIRECTIONAL, adj_max_freq=0, want_root=True):
        """dedup_batch by Levenshtein distance (umi_dedup_batch_edit): one-word keys, umi_len <= 21; nmask may
        be None whatever the keys hold.  An indel costs 2 between UMIs of one length, so the result differs
        from dedup_batch's from k = 2 on.  Returns (kept u8[N], root u32[N] or None, stats dict)."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        freq = np.ascontiguousarray(freq, dtype=np.int32)
        bucket_off = np.ascontiguousarray(bucket_off, dtype=np.uint64)
        nm = None if nmask is None else np.ascontiguousarray(nmask, dtype=np.uint64)
        n = len(keys)
        if len(freq) != n or (nm is not None and len(nm) != n):
            raise ValueError("keys/nmask/freq lengths differ")
        if len(bucket_off) < 1 or (len(bucket_off) > 1 and int(bucket_off[-1]) != n):
            raise ValueError("bucket_off[-1] must equal len(keys)")
        kept = np.zeros(n, dtype=np.uint8)
        root = np.zeros(n, dtype=np.uint32) if want_root else None
        st = Stats()
        check(load().umi_dedup_batch_edit(self._h, ptr(keys, C.c_uint64), ptr(nm, C.c_uint64),
                                          ptr(freq, C.c_int32), ptr(bucket_off, C.c_uint64),
                                          len(bucket_off) - 1, umi_len, k, percentage, algo,
                                          adj_max_freq, ptr(kept, C.c_uint8), ptr(root, C.c_uint32),
                                          C.byref(st)))
        return kept, root, st.as_dict()

    def dedup_batch_cr(self, keys, nmask, freq, bucket_off, umi_len, want_root=True, want_target=False):
        """Cell Ranger's one-mismatch correction (umi_dedup_batch_cr): every UMI goes to the best of itself and
        its one-mismatch neighbours by (count, string), and every target is a molecule -- not transitive, no k,
        no percentage.  One-word keys, umi_len <= 21; nmask may be None whatever the keys hold.  Returns
        (kept u8[N], root u32[N] or None, stats dict), with want_target (kept, root, target u32[N], stats)."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        freq = np.ascontiguousarray(freq, dtype=np.int32)
        bucket_off = np.ascontiguousarray(bucket_off, dtype=np.uint64)
        nm = None if nmask is None else np.ascontiguousarray(nmask, dtype=np.uint64)
        n = len(keys)
        if len(freq) != n or (nm is not None and len(nm) != n):
            raise ValueError("keys/nmask/freq lengths differ")
        if len(bucket_off) < 1 or (len(bucket_off) > 1 and int(bucket_off[-1]) != n):
            raise ValueError("bucket_off[-1] must equal len(keys)")
        kept = np.zeros(n, dtype=np.uint8)
        root = np.zeros(n, dtype=np.uint32) if want_root else None
        target = np.zeros(n, dtype=np.uint32) if want_target else None
        st = Stats()
        check(load().umi_dedup_batch_cr(self._h, ptr(keys, C.c_uint64), ptr(nm, C.c_uint64), ptr(freq, C.c_int32),
                                        ptr(bucket_off, C.c_uint64), len(bucket_off) - 1, umi_len,
                                        ptr(kept, C.c_uint8), ptr(root, C.c_uint32), ptr(target, C.c_uint32),
                                        C.byref(st)))
        if want_target:
            return kept, root, target, st.as_dict()
        return kept, root, st.as_dict()

    def dedup_batch_wide(self, keys, nmask, freq, bucket_off, umi_len, k=1, percentage=0.5,
                         algo=UMI_ALGO_DIRECTIONAL, adj_max_freq=0, want_root=True):
        """Batched call for keys of several words (umi_len > 21): keys / nmask uint64 [N, n_words]."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        n, w = keys.shape
        nm = None if nmask is None else np.ascontiguousarray(nmask, dtype=np.uint64)
        freq = np.ascontiguousarray(freq, dtype=np.int32)
        bucket_off = np.ascontiguousarray(bucket_off, dtype=np.uint64)
        kept = np.zeros(max(1, n), dtype=np.uint8)
        root = np.zeros(max(1, n), dtype=np.uint32) if want_root else None
        st = Stats()
        check(load().umi_dedup_batch_wide(self._h, ptr(keys, C.c_uint64), ptr(nm, C.c_uint64), w,
                                          ptr(freq, C.c_int32), ptr(bucket_off, C.c_uint64), len(bucket_off) - 1,
                                          umi_len, k, percentage, algo, adj_max_freq, ptr(kept, C.c_uint8),
                                          ptr(root, C.c_uint32), C.byref(st)))
        return kept[:n], (root[:n] if want_root else None), st.as_dict()

    def dedup_seqs(self, keys, nmask, freq, bucket_off, bucket_len, k=1, percentage=0.5,
                   algo=UMI_ALGO_DIRECTIONAL, adj_max_freq=0, want_root=True):
        """Whole reads as keys (umi_dedup_seqs): keys / nmask uint64 [N, n_words], bucket b of
        bucket_len[b] bases owns entries [bucket_off[b], bucket_off[b + 1]), several lengths in one call.
        Returns (kept u8[N], root u32[N] or None, stats dict)."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        if keys.ndim != 2:
            raise ValueError("keys must be [N, n_words]")
        n, w = keys.shape
        nm = None if nmask is None else np.ascontiguousarray(nmask, dtype=np.uint64)
        if nm is not None and nm.shape != keys.shape:
            raise ValueError("nmask must have the shape of keys")
        freq = np.ascontiguousarray(freq, dtype=np.int32)
        bucket_off = np.ascontiguousarray(bucket_off, dtype=np.uint64)
        bucket_len = np.ascontiguousarray(bucket_len, dtype=np.int32)
        if len(freq) != n or len(bucket_len) != len(bucket_off) - 1:
            raise ValueError("freq / bucket_len lengths differ from keys / bucket_off")
        if len(bucket_off) < 1 or (len(bucket_off) > 1 and int(bucket_off[-1]) != n):
            raise ValueError("bucket_off[-1] must equal len(keys)")
        kept = np.zeros(max(1, n), dtype=np.uint8)
        root = np.zeros(max(1, n), dtype=np.uint32) if want_root else None
        st = Stats()
        check(load().umi_dedup_seqs(self._h, ptr(keys, C.c_uint64), ptr(nm, C.c_uint64), w, ptr(freq, C.c_int32),
                                    ptr(bucket_off, C.c_uint64), ptr(bucket_len, C.c_int32), len(bucket_off) - 1, k,
                                    percentage, algo, adj_max_freq, ptr(kept, C.c_uint8), ptr(root, C.c_uint32),
                                    C.byref(st)))
        return kept[:n], (root[:n] if want_root else None), st.as_dict()

    def stage_seqs(self, seqs, quals=None, merge=1, n_words=None):
        """Staging of whole reads on the device (umi_stage_seqs): lists of bytes (reads, and their
        qualities for merge 1) in file order -> dict(keys, nmask [n_entries, n_words], freq, rep,
        entry_of_read, bucket_off, bucket_len, any_n), the input of dedup_seqs.  n_words =
        ceil(3 * longest / 64) unless given."""
        bs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
        n = len(bs)
        if quals is not None:
            qs = [q.encode() if isinstance(q, str) else bytes(q) for q in quals]
            if len(qs) != n or any(len(a) != len(b) for a, b in zip(bs, qs)):
                raise ValueError("quals must match seqs read by read")
        elif merge:
            raise ValueError("merge 1 needs quals")
        lens = np.array([len(b) for b in bs], dtype=np.uint32)
        if n_words is None:
            n_words = max(1, (3 * int(lens.max() if n else 0) + 63) // 64)
        text = b"".join(bs) + (b"".join(qs) if quals is not None else b"")
        seq_pos = np.zeros(n, dtype=np.uint64)
        if n:
            seq_pos[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
        qual_pos = seq_pos + np.uint64(sum(map(len, bs))) if quals is not None else None
        buf = np.frombuffer(text or b"\0", dtype=np.uint8)
        m = max(1, n)
        keys, nm = np.zeros((m, n_words), np.uint64), np.zeros((m, n_words), np.uint64)
        freq, rep, eor = np.zeros(m, np.int32), np.zeros(m, np.uint64), np.zeros(m, np.uint32)
        boff, blen = np.zeros(m + 1, np.uint64), np.zeros(m, np.int32)
        ne, nb, any_n = C.c_uint64(0), C.c_uint64(0), C.c_int(0)
        check(load().umi_stage_seqs(self._h, ptr(buf, C.c_uint8), ptr(seq_pos, C.c_uint64), ptr(qual_pos, C.c_uint64),
                                    ptr(lens, C.c_uint32), n, n_words, merge, ptr(keys, C.c_uint64), ptr(nm, C.c_uint64),
                                    ptr(freq, C.c_int32), ptr(rep, C.c_uint64), ptr(eor, C.c_uint32),
                                    ptr(boff, C.c_uint64), ptr(blen, C.c_int32), C.byref(ne), C.byref(nb),
                                    C.byref(any_n)))
        e, b = int(ne.value), int(nb.value)
        return dict(keys=keys[:e], nmask=nm[:e], freq=freq[:e], rep=rep[:e], entry_of_read=eor[:n],
                    bucket_off=boff[:b + 1], bucket_len=blen[:b], any_n=bool(any_n.value))

    def stage_seqs_device(self, d_text, d_seq_pos, d_qual_pos, d_len, n_reads, n_words, d_keys, d_nmask, d_freq,
                          d_rep, d_entry_of_read=0, merge=1, stream=0):
        """The same with the per-read and per-entry arrays in device memory (raw pointers); returns
        (bucket_off, bucket_len, n_entries, any_n), the bucket table on the host."""
        m = max(1, min(int(n_reads), 257))
        boff, blen = np.zeros(m + 1, np.uint64), np.zeros(m, np.int32)
        ne, nb, any_n = C.c_uint64(0), C.c_uint64(0), C.c_int(0)
        check(load().umi_stage_seqs_device(self._h, d_text, d_seq_pos, d_qual_pos or None, d_len, n_reads, n_words,
                                           merge, d_keys, d_nmask or None, d_freq, d_rep, d_entry_of_read or None,
                                           ptr(boff, C.c_uint64), ptr(blen, C.c_int32), C.byref(ne), C.byref(nb),
                                           C.byref(any_n), stream or None))
        b = int(nb.value)
        return boff[:b + 1], blen[:b], int(ne.value), bool(any_n.value)

    def consensus_seqs(self, seqs, quals, staged, kept, root):
        """One consensus read per cluster (umi_consensus_seqs): seqs / quals as given to stage_seqs,
        staged the dict it returned, kept / root from dedup_seqs.  Returns (cons_seqs, cons_quals,
        cluster_reads): lists of bytes and a uint32 array over the kept entries in ascending entry order."""
        bs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
        qs = [q.encode() if isinstance(q, str) else bytes(q) for q in quals]
        n = len(bs)
        if len(qs) != n or any(len(a) != len(b) for a, b in zip(bs, qs)):
            raise ValueError("quals must match seqs read by read")
        lens = np.array([len(b) for b in bs], dtype=np.uint32)
        total = int(lens.sum(dtype=np.uint64)) if n else 0
        seq_pos = np.zeros(max(1, n), dtype=np.uint64)
        if n:
            seq_pos[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
        qual_pos = seq_pos + np.uint64(total)
        buf = np.frombuffer((b"".join(bs) + b"".join(qs)) or b"\0", dtype=np.uint8)
        eor = np.ascontiguousarray(staged["entry_of_read"], dtype=np.uint32)
        freq = np.ascontiguousarray(staged["freq"], dtype=np.int32)
        boff = np.ascontiguousarray(staged["bucket_off"], dtype=np.uint64)
        blen = np.ascontiguousarray(staged["bucket_len"], dtype=np.int32)
        kept = np.ascontiguousarray(kept, dtype=np.uint8)
        root = np.ascontiguousarray(root, dtype=np.uint32)
        ne = len(freq)
        if len(eor) != n or len(kept) != ne or len(root) != ne or len(blen) != len(boff) - 1:
            raise ValueError("entry_of_read / kept / root / bucket table do not match the reads and entries")
        cons_seq, cons_qual = np.zeros(max(1, total), np.uint8), np.zeros(max(1, total), np.uint8)
        cons_off, cr = np.zeros(max(1, ne), np.uint64), np.zeros(max(1, ne), np.uint32)
        nbytes = C.c_uint64(0)
        check(load().umi_consensus_seqs(self._h, ptr(buf, C.c_uint8), ptr(seq_pos, C.c_uint64), ptr(qual_pos, C.c_uint64),
                                        ptr(lens, C.c_uint32), n, ptr(eor, C.c_uint32), ptr(freq, C.c_int32),
                                        ptr(kept, C.c_uint8), ptr(root, C.c_uint32), ne, ptr(boff, C.c_uint64),
                                        ptr(blen, C.c_int32), len(boff) - 1, ptr(cons_seq, C.c_uint8),
                                        ptr(cons_qual, C.c_uint8), ptr(cons_off, C.c_uint64), ptr(cr, C.c_uint32),
                                        C.byref(nbytes)))
        ks = np.flatnonzero(kept[:ne])
        bucket_of = np.searchsorted(boff, ks, side="right") - 1
        sb, qb = cons_seq.tobytes(), cons_qual.tobytes()
        out_s, out_q = [], []
        for r, b in zip(ks, bucket_of):
            o, L = int(cons_off[r]), int(blen[b])
            out_s.append(sb[o:o + L])
            out_q.append(qb[o:o + L])
        return out_s, out_q, cr[ks]

    def consensus_seqs_device(self, d_text, d_seq_pos, d_qual_pos, d_len, n_reads, d_entry_of_read, d_freq, d_kept,
                              d_root, n_entries, bucket_off, bucket_len, d_cons_seq, d_cons_qual, d_cons_off,
                              d_cluster_reads=0, stream=0):
        """The same on raw device pointers (umi_consensus_seqs_device; the bucket table stays on the host):
        fills d_cons_seq / d_cons_qual / d_cons_off / d_cluster_reads and returns the consensus bytes written."""
        boff = np.ascontiguousarray(bucket_off, dtype=np.uint64)
        blen = np.ascontiguousarray(bucket_len, dtype=np.int32)
        nbytes = C.c_uint64(0)
        check(load().umi_consensus_seqs_device(self._h, d_text, d_seq_pos, d_qual_pos or None, d_len, n_reads,
                                               d_entry_of_read, d_freq, d_kept, d_root, n_entries, ptr(boff, C.c_uint64),
                                               ptr(blen, C.c_int32), len(boff) - 1, d_cons_seq, d_cons_qual, d_cons_off,
                                               d_cluster_reads or None, C.byref(nbytes), stream or None))
        return int(nbytes.value)

    def consensus_bam(self, data, seq_pos, qual_pos, lens, cluster, cluster_len, want_disagree=True):
        """One consensus per cluster of aligned reads (umi_consensus_bam): read i is lens[i] bases packed two per
        byte at data[seq_pos[i]:], its Phred bytes at data[qual_pos[i]:]; cluster[i] is its cluster or
        UMI_NO_CLUSTER; cluster_len the clusters' lengths.  Returns (cons_seqs, cons_quals, depth, disagree):
        lists of bytes (packed sequence, qualities) and uint32 arrays over the clusters (disagree None if not
        wanted)."""
        buf = np.frombuffer(bytes(data) or b"\0", dtype=np.uint8)
        seq_pos = np.ascontiguousarray(seq_pos, dtype=np.uint64)
        qual_pos = np.ascontiguousarray(qual_pos, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        cluster = np.ascontiguousarray(cluster, dtype=np.uint32)
        clen = np.ascontiguousarray(cluster_len, dtype=np.uint32)
        n, nc = len(lens), len(clen)
        if len(seq_pos) != n or len(qual_pos) != n or len(cluster) != n:
            raise ValueError("seq_pos / qual_pos / lens / cluster lengths differ")
        fit = np.minimum(clen, _lib.UMI_MAX_CONS_LEN).astype(np.uint64)
        cons_seq = np.zeros(max(1, int(((fit + 1) // 2).sum())), np.uint8)
        cons_qual = np.zeros(max(1, int(fit.sum())), np.uint8)
        seq_off, qual_off = np.zeros(max(1, nc), np.uint64), np.zeros(max(1, nc), np.uint64)
        depth = np.zeros(max(1, nc), np.uint32)
        disagree = np.zeros(max(1, nc), np.uint32) if want_disagree else None
        sb, qb = C.c_uint64(0), C.c_uint64(0)
        check(load().umi_consensus_bam(self._h, ptr(buf, C.c_uint8), ptr(seq_pos, C.c_uint64), ptr(qual_pos, C.c_uint64),
                                       ptr(lens, C.c_uint32), ptr(cluster, C.c_uint32), n, ptr(clen, C.c_uint32), nc,
                                       ptr(cons_seq, C.c_uint8), ptr(cons_qual, C.c_uint8), ptr(seq_off, C.c_uint64),
                                       ptr(qual_off, C.c_uint64), ptr(depth, C.c_uint32), ptr(disagree, C.c_uint32),
                                       C.byref(sb), C.byref(qb)))
        s, q = cons_seq.tobytes(), cons_qual.tobytes()
        out_s = [s[int(seq_off[c]):int(seq_off[c]) + (int(clen[c]) + 1) // 2] for c in range(nc)]
        out_q = [q[int(qual_off[c]):int(qual_off[c]) + int(clen[c])] for c in range(nc)]
        return out_s, out_q, depth[:nc], (disagree[:nc] if want_disagree else None)

    def consensus_bam_device(self, d_data, d_seq_pos, d_qual_pos, d_len, d_cluster, n_reads, d_cluster_len, n_clusters,
                             d_cons_seq, d_cons_qual, d_seq_off, d_qual_off, d_depth, d_disagree=0, stream=0):
        """The same on raw device pointers (umi_consensus_bam_device): fills d_cons_seq / d_cons_qual / d_seq_off /
        d_qual_off / d_depth / d_disagree and returns (sequence bytes, quality bytes) written."""
        sb, qb = C.c_uint64(0), C.c_uint64(0)
        check(load().umi_consensus_bam_device(self._h, d_data or None, d_seq_pos or None, d_qual_pos or None, d_len or None,
                                              d_cluster or None, n_reads, d_cluster_len or None, n_clusters,
                                              d_cons_seq or None, d_cons_qual or None, d_seq_off or None, d_qual_off or None,
                                              d_depth or None, d_disagree or None, C.byref(sb), C.byref(qb), stream or None))
        return int(sb.value), int(qb.value)

    @staticmethod
    def _whitelist_bytes(whitelist, umi_len):
        """A list of str/bytes, or a uint8 array [n_wl * umi_len] -> (uint8 array, n_wl)."""
        if isinstance(whitelist, np.ndarray):
            wl = np.ascontiguousarray(whitelist, dtype=np.uint8).reshape(-1)
        else:
            bs = [w.encode() if isinstance(w, str) else bytes(w) for w in whitelist]
            if any(len(b) != umi_len for b in bs):
                raise ValueError("every listed UMI has umi_len bases")
            wl = np.frombuffer(b"".join(bs), dtype=np.uint8)
        if wl.size % umi_len:
            raise ValueError("the whitelist is not a whole number of UMIs")
        return wl, wl.size // umi_len

    def correct_umis(self, umi_bytes, umi_len, whitelist, max_mismatches=1, min_distance=1):
        """UMIs snapped to a fixed list (umi_correct_umis): umi_bytes uint8 [n * umi_len], whitelist a list of
        str/bytes or a uint8 array.  Returns dict(out uint8 [n * umi_len], match int32 [n] (-1: not matched),
        best, second uint8 [n], counts uint64 [3]: exact, corrected, unmatched)."""
        umi_bytes = np.ascontiguousarray(umi_bytes, dtype=np.uint8).reshape(-1)
        if umi_len < 1 or umi_bytes.size % umi_len:
            raise ValueError("umi_bytes is not a whole number of UMIs")
        n = umi_bytes.size // umi_len
        wl, n_wl = self._whitelist_bytes(whitelist, umi_len)
        m = max(1, n)
        out = np.zeros(m * umi_len, np.uint8)
        match = np.zeros(m, np.int32)
        best, second = np.zeros(m, np.uint8), np.zeros(m, np.uint8)
        counts = np.zeros(3, np.uint64)
        check(load().umi_correct_umis(self._h, ptr(umi_bytes, C.c_uint8), n, umi_len, ptr(wl, C.c_uint8), n_wl,
                                      max_mismatches, min_distance, ptr(out, C.c_uint8), ptr(match, C.c_int32),
                                      ptr(best, C.c_uint8), ptr(second, C.c_uint8), ptr(counts, C.c_uint64)))
        return {"out": out[:n * umi_len], "match": match[:n], "best": best[:n], "second": second[:n], "counts": counts}

    def correct_umis_device(self, d_umi, n_reads, umi_len, whitelist, max_mismatches, min_distance, d_out, d_match,
                            d_best=0, d_second=0, stream=0):
        """The same on raw device pointers (umi_correct_umis_device; the whitelist stays on the host): fills
        d_match and, where given, d_out (may be d_umi) / d_best / d_second; returns counts uint64 [3]."""
        wl, n_wl = self._whitelist_bytes(whitelist, umi_len)
        counts = np.zeros(3, np.uint64)
        check(load().umi_correct_umis_device(self._h, d_umi or None, n_reads, umi_len, ptr(wl, C.c_uint8), n_wl,
                                             max_mismatches, min_distance, d_out or None, d_match or None,
                                             d_best or None, d_second or None, ptr(counts, C.c_uint64), stream or None))
        return counts

    def correct_barcodes(self, bc_bytes, bc_len, whitelist, max_mismatches=1):
        """Cell barcodes snapped to a kit's list by an indexed lookup (umi_correct_barcodes): bc_bytes uint8
        [n * bc_len], whitelist a list of str/bytes or a uint8 array, without duplicates.  Returns dict(match
        int32 [n] (-1: none or ambiguous), status uint8 [n] (0 exact, 1 corrected, 2 none, 3 ambiguous), counts
        uint64 [4], by status)."""
        bc_bytes = np.ascontiguousarray(bc_bytes, dtype=np.uint8).reshape(-1)
        if bc_len < 1 or bc_bytes.size % bc_len:
            raise ValueError("bc_bytes is not a whole number of barcodes")
        n = bc_bytes.size // bc_len
        wl, n_wl = self._whitelist_bytes(whitelist, bc_len)
        m = max(1, n)
        match, status = np.zeros(m, np.int32), np.zeros(m, np.uint8)
        counts = np.zeros(4, np.uint64)
        check(load().umi_correct_barcodes(self._h, ptr(bc_bytes, C.c_uint8), n, bc_len, ptr(wl, C.c_uint8), n_wl,
                                          max_mismatches, ptr(match, C.c_int32), ptr(status, C.c_uint8),
                                          ptr(counts, C.c_uint64)))
        return {"match": match[:n], "status": status[:n], "counts": counts}

    def correct_barcodes_device(self, d_bc, n_reads, bc_len, whitelist, max_mismatches, d_match, d_status=0, stream=0):
        """The same on raw device pointers (umi_correct_barcodes_device; the whitelist stays on the host): fills
        d_match and, where given, d_status; returns counts uint64 [4]."""
        wl, n_wl = self._whitelist_bytes(whitelist, bc_len)
        counts = np.zeros(4, np.uint64)
        check(load().umi_correct_barcodes_device(self._h, d_bc or None, n_reads, bc_len, ptr(wl, C.c_uint8), n_wl,
                                                 max_mismatches, d_match or None, d_status or None,
                                                 ptr(counts, C.c_uint64), stream or None))
        return counts

    def correct_barcodes_multi(self, bc_bytes, qual_bytes, bc_len, whitelist, min_posterior_permille=975, pseudocount=0):
        """correct_barcodes with max_mismatches 1 and the ambiguous reads decided by posterior
        (umi_correct_barcodes_multi): qual_bytes uint8 [n * bc_len], Phred + 33, beside bc_bytes.  A candidate's
        weight is (its exact reads in this call + pseudocount) times the chance of an error at the quality of the
        mismatched base; the heaviest is taken where it holds min_posterior_permille of all the weight.  Returns
        dict(match int32 [n], status uint8 [n] (... 3 ambiguous, 4 resolved), counts uint64 [5], exact_reads
        uint32 [n_wl])."""
        bc_bytes = np.ascontiguousarray(bc_bytes, dtype=np.uint8).reshape(-1)
        qual_bytes = np.ascontiguousarray(qual_bytes, dtype=np.uint8).reshape(-1)
        if bc_len < 1 or bc_bytes.size % bc_len:
            raise ValueError("bc_bytes is not a whole number of barcodes")
        if qual_bytes.size != bc_bytes.size:
            raise ValueError("qual_bytes is not of bc_bytes' size")
        n = bc_bytes.size // bc_len
        wl, n_wl = self._whitelist_bytes(whitelist, bc_len)
        m = max(1, n)
        match, status = np.zeros(m, np.int32), np.zeros(m, np.uint8)
        counts, exact_reads = np.zeros(5, np.uint64), np.zeros(max(1, n_wl), np.uint32)
        check(load().umi_correct_barcodes_multi(self._h, ptr(bc_bytes, C.c_uint8), ptr(qual_bytes, C.c_uint8), n, bc_len,
                                                ptr(wl, C.c_uint8), n_wl, min_posterior_permille, pseudocount,
                                                ptr(match, C.c_int32), ptr(status, C.c_uint8),
                                                ptr(exact_reads, C.c_uint32), ptr(counts, C.c_uint64)))
        return {"match": match[:n], "status": status[:n], "counts": counts, "exact_reads": exact_reads[:n_wl]}

    def correct_barcodes_multi_device(self, d_bc, d_qual, n_reads, bc_len, whitelist, min_posterior_permille, pseudocount,
                                      d_match, d_status=0, d_exact_reads=0, stream=0):
        """The same on raw device pointers (umi_correct_barcodes_multi_device; the whitelist stays on the host):
        fills d_match and, where given, d_status and d_exact_reads (uint32 [n_wl]); returns counts uint64 [5]."""
        wl, n_wl = self._whitelist_bytes(whitelist, bc_len)
        counts = np.zeros(5, np.uint64)
        check(load().umi_correct_barcodes_multi_device(self._h, d_bc or None, d_qual or None, n_reads, bc_len,
                                                       ptr(wl, C.c_uint8), n_wl, min_posterior_permille, pseudocount,
                                                       d_match or None, d_status or None, d_exact_reads or None,
                                                       ptr(counts, C.c_uint64), stream or None))
        return counts

    @staticmethod
    def _exon_arrays(exons):
        """exons: a dict of ref, start, end, gene (int32) and strand (uint8, the ASCII bytes of + - .), or a
        sequence of (ref, start, end, strand, gene) with strand a one-letter str"""
        if not isinstance(exons, dict):
            rows = list(exons)
            exons = {"ref": [e[0] for e in rows], "start": [e[1] for e in rows], "end": [e[2] for e in rows],
                     "strand": np.frombuffer("".join(e[3] for e in rows).encode("latin-1"), np.uint8),
                     "gene": [e[4] for e in rows]}
        a = [np.ascontiguousarray(exons[k], dtype=np.uint8 if k == "strand" else np.int32).reshape(-1)
             for k in ("ref", "start", "end", "strand", "gene")]
        if len({len(x) for x in a}) != 1:
            raise ValueError("the exon arrays differ in length")
        return a

    def assign_genes(self, exons, n_genes, strand_mode, read_ref, read_pos, read_reverse, cigar, cigar_off):
        """Reads assigned to genes from an annotation by featureCounts' default rule (umi_assign_genes; the rule is
        in include/umihip.h): exons as _exon_arrays takes them, strand_mode one of UMI_STRAND_*, per read its
        reference, 0-based position, strand (not 0: reverse) and CIGAR words cigar[cigar_off[i]:cigar_off[i + 1]]
        (BAM's, len << 4 | op).  Returns dict(gene int32 [n] (-1 unless assigned), status uint8 [n] (0 assigned,
        1 none, 2 several), counts uint64 [3], by status)."""
        ex = self._exon_arrays(exons)
        read_ref = np.ascontiguousarray(read_ref, dtype=np.int32).reshape(-1)
        read_pos = np.ascontiguousarray(read_pos, dtype=np.int32).reshape(-1)
        read_reverse = np.ascontiguousarray(read_reverse, dtype=np.uint8).reshape(-1)
        cigar = np.ascontiguousarray(cigar, dtype=np.uint32).reshape(-1)
        cigar_off = np.ascontiguousarray(cigar_off, dtype=np.uint64).reshape(-1)
        n = len(read_ref)
        if len(read_pos) != n or len(read_reverse) != n or len(cigar_off) != n + 1:
            raise ValueError("the read arrays differ in length (cigar_off has one entry more)")
        if int(cigar_off[-1]) > len(cigar):
            raise ValueError("cigar_off ends beyond cigar")
        m = max(1, n)
        gene, status = np.zeros(m, np.int32), np.zeros(m, np.uint8)
        counts = np.zeros(3, np.uint64)
        check(load().umi_assign_genes(self._h, ptr(ex[0], C.c_int32), ptr(ex[1], C.c_int32), ptr(ex[2], C.c_int32),
                                      ptr(ex[3], C.c_uint8), ptr(ex[4], C.c_int32), len(ex[0]), n_genes, strand_mode,
                                      ptr(read_ref, C.c_int32), ptr(read_pos, C.c_int32), ptr(read_reverse, C.c_uint8),
                                      ptr(cigar, C.c_uint32), ptr(cigar_off, C.c_uint64), n, ptr(gene, C.c_int32),
                                      ptr(status, C.c_uint8), ptr(counts, C.c_uint64)))
        return {"gene": gene[:n], "status": status[:n], "counts": counts}

    def assign_genes_device(self, exons, n_genes, strand_mode, d_read_ref, d_read_pos, d_read_reverse, d_cigar, d_cigar_off,
                            n_reads, d_gene, d_status, stream=0):
        """The same on raw device pointers (umi_assign_genes_device; the exons stay on the host): fills d_gene
        (int32 [n_reads]) and d_status (uint8 [n_reads]); returns counts uint64 [3]."""
        ex = self._exon_arrays(exons)
        counts = np.zeros(3, np.uint64)
        check(load().umi_assign_genes_device(self._h, ptr(ex[0], C.c_int32), ptr(ex[1], C.c_int32), ptr(ex[2], C.c_int32),
                                             ptr(ex[3], C.c_uint8), ptr(ex[4], C.c_int32), len(ex[0]), n_genes,
                                             strand_mode, d_read_ref or None, d_read_pos or None, d_read_reverse or None,
                                             d_cigar or None, d_cigar_off or None, n_reads, d_gene or None,
                                             d_status or None, ptr(counts, C.c_uint64), stream or None))
        return counts

    @staticmethod
    def _transcript_array(exons, n_exons):
        """exon_transcript of exons: the dict's "transcript", or the sixth element of every tuple"""
        tr = exons["transcript"] if isinstance(exons, dict) else [e[5] for e in exons]
        tr = np.ascontiguousarray(tr, dtype=np.int32).reshape(-1)
        if len(tr) != n_exons:
            raise ValueError("the exon arrays differ in length")
        return tr

    def assign_genes_transcripts(self, exons, n_genes, n_transcripts, strand_mode, read_ref, read_pos, read_reverse, cigar,
                                 cigar_off):
        """Reads assigned to genes by transcript model, STARsolo's Gene (umi_assign_genes_transcripts; the rule is in
        include/umihip.h): assign_genes' arguments, the exons with their transcript -- a dict with "transcript" (int32)
        beside _exon_arrays' keys, or (ref, start, end, strand, gene, transcript) tuples -- and n_transcripts.  Returns
        assign_genes' dict."""
        exons = exons if isinstance(exons, dict) else list(exons)
        ex = self._exon_arrays(exons)
        tr = self._transcript_array(exons, len(ex[0]))
        read_ref = np.ascontiguousarray(read_ref, dtype=np.int32).reshape(-1)
        read_pos = np.ascontiguousarray(read_pos, dtype=np.int32).reshape(-1)
        read_reverse = np.ascontiguousarray(read_reverse, dtype=np.uint8).reshape(-1)
        cigar = np.ascontiguousarray(cigar, dtype=np.uint32).reshape(-1)
        cigar_off = np.ascontiguousarray(cigar_off, dtype=np.uint64).reshape(-1)
        n = len(read_ref)
        if len(read_pos) != n or len(read_reverse) != n or len(cigar_off) != n + 1:
            raise ValueError("the read arrays differ in length (cigar_off has one entry more)")
        if int(cigar_off[-1]) > len(cigar):
            raise ValueError("cigar_off ends beyond cigar")
        m = max(1, n)
        gene, status = np.zeros(m, np.int32), np.zeros(m, np.uint8)
        counts = np.zeros(3, np.uint64)
        check(load().umi_assign_genes_transcripts(self._h, ptr(ex[0], C.c_int32), ptr(ex[1], C.c_int32), ptr(ex[2], C.c_int32),
                                                  ptr(ex[3], C.c_uint8), ptr(ex[4], C.c_int32), ptr(tr, C.c_int32), len(ex[0]),
                                                  n_genes, n_transcripts, strand_mode, ptr(read_ref, C.c_int32),
                                                  ptr(read_pos, C.c_int32), ptr(read_reverse, C.c_uint8), ptr(cigar, C.c_uint32),
                                                  ptr(cigar_off, C.c_uint64), n, ptr(gene, C.c_int32), ptr(status, C.c_uint8),
                                                  ptr(counts, C.c_uint64)))
        return {"gene": gene[:n], "status": status[:n], "counts": counts}

    def assign_genes_transcripts_device(self, exons, n_genes, n_transcripts, strand_mode, d_read_ref, d_read_pos, d_read_reverse,
                                        d_cigar, d_cigar_off, n_reads, d_gene, d_status, stream=0):
        """The same on raw device pointers (umi_assign_genes_transcripts_device; the exons stay on the host): fills
        d_gene (int32 [n_reads]) and d_status (uint8 [n_reads]); returns counts uint64 [3]."""
        exons = exons if isinstance(exons, dict) else list(exons)
        ex = self._exon_arrays(exons)
        tr = self._transcript_array(exons, len(ex[0]))
        counts = np.zeros(3, np.uint64)
        check(load().umi_assign_genes_transcripts_device(self._h, ptr(ex[0], C.c_int32), ptr(ex[1], C.c_int32),
                                                         ptr(ex[2], C.c_int32), ptr(ex[3], C.c_uint8), ptr(ex[4], C.c_int32),
                                                         ptr(tr, C.c_int32), len(ex[0]), n_genes, n_transcripts, strand_mode,
                                                         d_read_ref or None, d_read_pos or None, d_read_reverse or None,
                                                         d_cigar or None, d_cigar_off or None, n_reads, d_gene or None,
                                                         d_status or None, ptr(counts, C.c_uint64), stream or None))
        return counts

    def assign_genes_introns(self, exons, n_genes, strand_mode, intron_mode, read_ref, read_pos, read_reverse, cigar, cigar_off):
        """Reads assigned to genes with their introns (umi_assign_genes_introns; the rule is in include/umihip.h):
        assign_genes' arguments and intron_mode, one of UMI_INTRONS_*.  Returns dict(gene int32 [n] (-1 unless
        assigned), status uint8 [n] (0 assigned, 1 none, 2 several), tier uint8 [n] (0 exon, 1 intron; 0 unless
        assigned), counts uint64 [4]: assigned by an exon, by an intron, none, several)."""
        ex = self._exon_arrays(exons)
        read_ref = np.ascontiguousarray(read_ref, dtype=np.int32).reshape(-1)
        read_pos = np.ascontiguousarray(read_pos, dtype=np.int32).reshape(-1)
        read_reverse = np.ascontiguousarray(read_reverse, dtype=np.uint8).reshape(-1)
        cigar = np.ascontiguousarray(cigar, dtype=np.uint32).reshape(-1)
        cigar_off = np.ascontiguousarray(cigar_off, dtype=np.uint64).reshape(-1)
        n = len(read_ref)
        if len(read_pos) != n or len(read_reverse) != n or len(cigar_off) != n + 1:
            raise ValueError("the read arrays differ in length (cigar_off has one entry more)")
        if int(cigar_off[-1]) > len(cigar):
            raise ValueError("cigar_off ends beyond cigar")
        m = max(1, n)
        gene, status, tier = np.zeros(m, np.int32), np.zeros(m, np.uint8), np.zeros(m, np.uint8)
        counts = np.zeros(4, np.uint64)
        check(load().umi_assign_genes_introns(self._h, ptr(ex[0], C.c_int32), ptr(ex[1], C.c_int32), ptr(ex[2], C.c_int32),
                                              ptr(ex[3], C.c_uint8), ptr(ex[4], C.c_int32), len(ex[0]), n_genes, strand_mode,
                                              intron_mode, ptr(read_ref, C.c_int32), ptr(read_pos, C.c_int32),
                                              ptr(read_reverse, C.c_uint8), ptr(cigar, C.c_uint32), ptr(cigar_off, C.c_uint64),
                                              n, ptr(gene, C.c_int32), ptr(status, C.c_uint8), ptr(tier, C.c_uint8),
                                              ptr(counts, C.c_uint64)))
        return {"gene": gene[:n], "status": status[:n], "tier": tier[:n], "counts": counts}

    def assign_genes_introns_device(self, exons, n_genes, strand_mode, intron_mode, d_read_ref, d_read_pos, d_read_reverse,
                                    d_cigar, d_cigar_off, n_reads, d_gene, d_status, d_tier, stream=0):
        """The same on raw device pointers (umi_assign_genes_introns_device; the exons stay on the host): fills
        d_gene (int32 [n_reads]), d_status and d_tier (uint8 [n_reads]); returns counts uint64 [4]."""
        ex = self._exon_arrays(exons)
        counts = np.zeros(4, np.uint64)
        check(load().umi_assign_genes_introns_device(self._h, ptr(ex[0], C.c_int32), ptr(ex[1], C.c_int32),
                                                     ptr(ex[2], C.c_int32), ptr(ex[3], C.c_uint8), ptr(ex[4], C.c_int32),
                                                     len(ex[0]), n_genes, strand_mode, intron_mode, d_read_ref or None,
                                                     d_read_pos or None, d_read_reverse or None, d_cigar or None,
                                                     d_cigar_off or None, n_reads, d_gene or None, d_status or None,
                                                     d_tier or None, ptr(counts, C.c_uint64), stream or None))
        return counts

    def assign_genes_classes(self, exons, n_genes, strand_mode, intron_mode, read_ref, read_pos, read_reverse, cigar, cigar_off):
        """Reads assigned to genes with their introns, and the class of every assigned read (umi_assign_genes_classes;
        the rule is in include/umihip.h): assign_genes_introns' arguments.  Returns its dict and, beside it, cls uint8
        [n] (UMI_READ_CLASS_*: 0 none, 1 exonic, 2 junction, 3 spanning, 4 intronic) and class_counts uint64 [5]."""
        ex = self._exon_arrays(exons)
        read_ref = np.ascontiguousarray(read_ref, dtype=np.int32).reshape(-1)
        read_pos = np.ascontiguousarray(read_pos, dtype=np.int32).reshape(-1)
        read_reverse = np.ascontiguousarray(read_reverse, dtype=np.uint8).reshape(-1)
        cigar = np.ascontiguousarray(cigar, dtype=np.uint32).reshape(-1)
        cigar_off = np.ascontiguousarray(cigar_off, dtype=np.uint64).reshape(-1)
        n = len(read_ref)
        if len(read_pos) != n or len(read_reverse) != n or len(cigar_off) != n + 1:
            raise ValueError("the read arrays differ in length (cigar_off has one entry more)")
        if int(cigar_off[-1]) > len(cigar):
            raise ValueError("cigar_off ends beyond cigar")
        m = max(1, n)
        gene, status, tier, cls = np.zeros(m, np.int32), np.zeros(m, np.uint8), np.zeros(m, np.uint8), np.zeros(m, np.uint8)
        counts, class_counts = np.zeros(4, np.uint64), np.zeros(5, np.uint64)
        check(load().umi_assign_genes_classes(self._h, ptr(ex[0], C.c_int32), ptr(ex[1], C.c_int32), ptr(ex[2], C.c_int32),
                                              ptr(ex[3], C.c_uint8), ptr(ex[4], C.c_int32), len(ex[0]), n_genes, strand_mode,
                                              intron_mode, ptr(read_ref, C.c_int32), ptr(read_pos, C.c_int32),
                                              ptr(read_reverse, C.c_uint8), ptr(cigar, C.c_uint32), ptr(cigar_off, C.c_uint64),
                                              n, ptr(gene, C.c_int32), ptr(status, C.c_uint8), ptr(tier, C.c_uint8),
                                              ptr(cls, C.c_uint8), ptr(counts, C.c_uint64), ptr(class_counts, C.c_uint64)))
        return {"gene": gene[:n], "status": status[:n], "tier": tier[:n], "cls": cls[:n], "counts": counts,
                "class_counts": class_counts}

    def assign_genes_classes_device(self, exons, n_genes, strand_mode, intron_mode, d_read_ref, d_read_pos, d_read_reverse,
                                    d_cigar, d_cigar_off, n_reads, d_gene, d_status, d_tier, d_cls, stream=0):
        """The same on raw device pointers (umi_assign_genes_classes_device; the exons stay on the host): fills d_gene
        (int32 [n_reads]), d_status, d_tier and d_cls (uint8 [n_reads]); returns (counts uint64 [4], class_counts
        uint64 [5])."""
        ex = self._exon_arrays(exons)
        counts, class_counts = np.zeros(4, np.uint64), np.zeros(5, np.uint64)
        check(load().umi_assign_genes_classes_device(self._h, ptr(ex[0], C.c_int32), ptr(ex[1], C.c_int32),
                                                     ptr(ex[2], C.c_int32), ptr(ex[3], C.c_uint8), ptr(ex[4], C.c_int32),
                                                     len(ex[0]), n_genes, strand_mode, intron_mode, d_read_ref or None,
                                                     d_read_pos or None, d_read_reverse or None, d_cigar or None,
                                                     d_cigar_off or None, n_reads, d_gene or None, d_status or None,
                                                     d_tier or None, d_cls or None, ptr(counts, C.c_uint64),
                                                     ptr(class_counts, C.c_uint64), stream or None))
        return counts, class_counts

    def assign_genes_transcripts_classes(self, exons, n_genes, n_transcripts, strand_mode, intron_mode, read_ref, read_pos,
                                         read_reverse, cigar, cigar_off, classes=True):
        """Reads assigned to genes by transcript model, with the gene bodies behind it and the class of every assigned
        read (umi_assign_genes_transcripts_classes; the rule is in include/umihip.h): assign_genes_transcripts' arguments
        and intron_mode, one of UMI_INTRONS_*.  Returns assign_genes_classes' dict; counts: assigned by a transcript, by a
        body, none, several.  classes=False: no class is computed, and the dict has neither cls nor class_counts."""
        exons = exons if isinstance(exons, dict) else list(exons)
        ex = self._exon_arrays(exons)
        tr = self._transcript_array(exons, len(ex[0]))
        read_ref = np.ascontiguousarray(read_ref, dtype=np.int32).reshape(-1)
        read_pos = np.ascontiguousarray(read_pos, dtype=np.int32).reshape(-1)
        read_reverse = np.ascontiguousarray(read_reverse, dtype=np.uint8).reshape(-1)
        cigar = np.ascontiguousarray(cigar, dtype=np.uint32).reshape(-1)
        cigar_off = np.ascontiguousarray(cigar_off, dtype=np.uint64).reshape(-1)
        n = len(read_ref)
        if len(read_pos) != n or len(read_reverse) != n or len(cigar_off) != n + 1:
            raise ValueError("the read arrays differ in length (cigar_off has one entry more)")
        if int(cigar_off[-1]) > len(cigar):
            raise ValueError("cigar_off ends beyond cigar")
        m = max(1, n)
        gene, status, tier, cls = np.zeros(m, np.int32), np.zeros(m, np.uint8), np.zeros(m, np.uint8), np.zeros(m, np.uint8)
        counts, class_counts = np.zeros(4, np.uint64), np.zeros(5, np.uint64)
        check(load().umi_assign_genes_transcripts_classes(
            self._h, ptr(ex[0], C.c_int32), ptr(ex[1], C.c_int32), ptr(ex[2], C.c_int32), ptr(ex[3], C.c_uint8), ptr(ex[4], C.c_int32),
            ptr(tr, C.c_int32), len(ex[0]), n_genes, n_transcripts, strand_mode, intron_mode, ptr(read_ref, C.c_int32),
            ptr(read_pos, C.c_int32), ptr(read_reverse, C.c_uint8), ptr(cigar, C.c_uint32), ptr(cigar_off, C.c_uint64), n,
            ptr(gene, C.c_int32), ptr(status, C.c_uint8), ptr(tier, C.c_uint8), ptr(cls, C.c_uint8) if classes else None,
            ptr(counts, C.c_uint64), ptr(class_counts, C.c_uint64) if classes else None))
        out = {"gene": gene[:n], "status": status[:n], "tier": tier[:n], "counts": counts}
        if classes:
            out["cls"], out["class_counts"] = cls[:n], class_counts
        return out

    def assign_genes_transcripts_classes_device(self, exons, n_genes, n_transcripts, strand_mode, intron_mode, d_read_ref,
                                                d_read_pos, d_read_reverse, d_cigar, d_cigar_off, n_reads, d_gene, d_status,
                                                d_tier, d_cls, stream=0, classes=True):
        """The same on raw device pointers (umi_assign_genes_transcripts_classes_device; the exons stay on the host): fills
        d_gene (int32 [n_reads]), d_status, d_tier and d_cls (uint8 [n_reads]); returns (counts uint64 [4], class_counts
        uint64 [5]).  classes=False: d_cls is not passed on and not written, and class_counts is None."""
        exons = exons if isinstance(exons, dict) else list(exons)
        ex = self._exon_arrays(exons)
        tr = self._transcript_array(exons, len(ex[0]))
        counts, class_counts = np.zeros(4, np.uint64), np.zeros(5, np.uint64) if classes else None
        check(load().umi_assign_genes_transcripts_classes_device(
            self._h, ptr(ex[0], C.c_int32), ptr(ex[1], C.c_int32), ptr(ex[2], C.c_int32), ptr(ex[3], C.c_uint8), ptr(ex[4], C.c_int32),
            ptr(tr, C.c_int32), len(ex[0]), n_genes, n_transcripts, strand_mode, intron_mode, d_read_ref or None, d_read_pos or None,
            d_read_reverse or None, d_cigar or None, d_cigar_off or None, n_reads, d_gene or None, d_status or None, d_tier or None,
            (d_cls or None) if classes else None, ptr(counts, C.c_uint64), ptr(class_counts, C.c_uint64) if classes else None,
            stream or None))
        return counts, class_counts

    def velocity_matrix(self, read_entry, read_class, kept, root, bucket_off, row, col, n_rows, n_cols):
        """Spliced, unspliced and ambiguous molecules per (column, row) pair (umi_velocity_matrix): read_entry uint32
        [n_reads] (UMI_READ_UNSTAGED: the read is skipped) and read_class uint8 [n_reads] (assign_genes_classes' cls),
        kept uint8 [N] and root uint32 [N] of a batched call, the buckets as count_matrix takes them.  Returns
        (out_row, out_col, spliced, unspliced, ambiguous), uint32, count_matrix's triplets in its order."""
        read_entry = np.ascontiguousarray(read_entry, dtype=np.uint32).reshape(-1)
        read_class = np.ascontiguousarray(read_class, dtype=np.uint8).reshape(-1)
        kept = np.ascontiguousarray(kept, dtype=np.uint8)
        root = np.ascontiguousarray(root, dtype=np.uint32)
        bucket_off = np.ascontiguousarray(bucket_off, dtype=np.uint64)
        row = np.ascontiguousarray(row, dtype=np.uint32)
        col = np.ascontiguousarray(col, dtype=np.uint32)
        nb = len(bucket_off) - 1
        if nb < 0 or len(row) != nb or len(col) != nb:
            raise ValueError("row / col want one element per bucket")
        if len(read_entry) != len(read_class):
            raise ValueError("read_entry / read_class lengths differ")
        if len(kept) != len(root) or (nb and int(bucket_off.max()) > len(kept)):
            raise ValueError("kept / root lengths differ, or bucket_off runs past them")
        m = max(1, nb)
        o_row, o_col, o_s, o_u, o_a = (np.zeros(m, np.uint32) for _ in range(5))
        nnz = C.c_uint64(0)
        check(load().umi_velocity_matrix(self._h, ptr(read_entry, C.c_uint32), ptr(read_class, C.c_uint8), len(read_entry),
                                         ptr(kept, C.c_uint8), ptr(root, C.c_uint32), ptr(bucket_off, C.c_uint64), nb,
                                         ptr(row, C.c_uint32), ptr(col, C.c_uint32), n_rows, n_cols, ptr(o_row, C.c_uint32),
                                         ptr(o_col, C.c_uint32), ptr(o_s, C.c_uint32), ptr(o_u, C.c_uint32),
                                         ptr(o_a, C.c_uint32), C.byref(nnz)))
        z = int(nnz.value)
        return o_row[:z], o_col[:z], o_s[:z], o_u[:z], o_a[:z]

    def velocity_matrix_device(self, d_read_entry, d_read_class, n_reads, d_kept, d_root, bucket_off, d_row, d_col, n_rows,
                               n_cols, d_out_row, d_out_col, d_out_spliced, d_out_unspliced, d_out_ambiguous, stream=0):
        """The same on raw device pointers (umi_velocity_matrix_device; bucket_off stays on the host): fills the five
        output arrays (room for n_buckets elements each) and returns nnz."""
        bucket_off = np.ascontiguousarray(bucket_off, dtype=np.uint64)
        nnz = C.c_uint64(0)
        check(load().umi_velocity_matrix_device(self._h, d_read_entry or None, d_read_class or None, n_reads, d_kept or None,
                                                d_root or None, ptr(bucket_off, C.c_uint64), len(bucket_off) - 1,
                                                d_row or None, d_col or None, n_rows, n_cols, d_out_row or None,
                                                d_out_col or None, d_out_spliced or None, d_out_unspliced or None,
                                                d_out_ambiguous or None, C.byref(nnz), stream or None))
        return int(nnz.value)

    def junction_matrix(self, read_ref, read_pos, cigar, cigar_off, read_entry, kept, root, bucket_off, col, n_cols,
                        capacity=None):
        """Molecules and reads per (column, splice junction) pair (umi_junction_matrix; the rule is in
        include/umihip.h): per read read_ref, read_pos (int32), its CIGAR words cigar[cigar_off[i] .. cigar_off[i + 1])
        and read_entry uint32 (UMI_READ_UNSTAGED: the read is skipped); kept uint8 [N] and root uint32 [N] of a batched
        call, bucket_off uint64 [n_buckets + 1], col uint32 [n_buckets].  capacity: the junction occurrences the outputs
        have room for (None: the N words among the CIGARs, an upper bound).  Returns ((jn_ref, jn_start, jn_end) int32,
        the junction table in the order of (ref, start, end); (out_jn, out_col, molecules uint32, reads uint64), sorted
        by column, then junction; counts uint64 [4]: spliced reads counted, occurrences, junctions, triplets).  The
        collapse is the call's own; nothing is collapsed again per junction, and a junction has no strand."""
        read_ref = np.ascontiguousarray(read_ref, dtype=np.int32).reshape(-1)
        read_pos = np.ascontiguousarray(read_pos, dtype=np.int32).reshape(-1)
        cigar = np.ascontiguousarray(cigar, dtype=np.uint32).reshape(-1)
        cigar_off = np.ascontiguousarray(cigar_off, dtype=np.uint64).reshape(-1)
        read_entry = np.ascontiguousarray(read_entry, dtype=np.uint32).reshape(-1)
        kept = np.ascontiguousarray(kept, dtype=np.uint8)
        root = np.ascontiguousarray(root, dtype=np.uint32)
        bucket_off = np.ascontiguousarray(bucket_off, dtype=np.uint64)
        col = np.ascontiguousarray(col, dtype=np.uint32)
        nb, nr = len(bucket_off) - 1, len(read_ref)
        if nb < 0 or len(col) != nb:
            raise ValueError("col wants one element per bucket")
        if len(read_pos) != nr or len(read_entry) != nr or len(cigar_off) != nr + 1:
            raise ValueError("read_ref / read_pos / read_entry / cigar_off lengths differ")
        if len(kept) != len(root) or (nb and int(bucket_off.max()) > len(kept)):
            raise ValueError("kept / root lengths differ, or bucket_off runs past them")
        if capacity is None:
            capacity = int(np.count_nonzero((cigar & 15) == 3))
        cap = max(1, int(capacity))
        if len(cigar) == 0:
            cigar = np.zeros(1, np.uint32)
        jn = [np.zeros(cap, np.int32) for _ in range(3)]
        o_jn, o_col, o_mol = (np.zeros(cap, np.uint32) for _ in range(3))
        o_reads = np.zeros(cap, np.uint64)
        counts = np.zeros(4, np.uint64)
        self.junction_counts = counts  # (what a refused call found: counts[1] = the occurrences a capacity has to hold)
        check(load().umi_junction_matrix(self._h, ptr(read_ref, C.c_int32), ptr(read_pos, C.c_int32), ptr(cigar, C.c_uint32),
                                         ptr(cigar_off, C.c_uint64), ptr(read_entry, C.c_uint32), nr, ptr(kept, C.c_uint8),
                                         ptr(root, C.c_uint32), ptr(bucket_off, C.c_uint64), nb, ptr(col, C.c_uint32), n_cols,
                                         int(capacity), ptr(jn[0], C.c_int32), ptr(jn[1], C.c_int32), ptr(jn[2], C.c_int32),
                                         ptr(o_jn, C.c_uint32), ptr(o_col, C.c_uint32), ptr(o_mol, C.c_uint32),
                                         ptr(o_reads, C.c_uint64), ptr(counts, C.c_uint64)))
        j, z = int(counts[2]), int(counts[3])
        return (jn[0][:j], jn[1][:j], jn[2][:j]), (o_jn[:z], o_col[:z], o_mol[:z], o_reads[:z]), counts

    def junction_matrix_device(self, d_read_ref, d_read_pos, d_cigar, d_cigar_off, d_read_entry, n_reads, d_kept, d_root,
                               bucket_off, d_col, n_cols, capacity, d_jn_ref, d_jn_start, d_jn_end, d_out_jn, d_out_col,
                               d_out_molecules, d_out_reads, stream=0):
        """The same on raw device pointers (umi_junction_matrix_device; bucket_off stays on the host): fills the seven
        output arrays (room for `capacity` elements each) and returns counts uint64 [4].  Where the call is refused,
        self.junction_counts[1] holds the occurrences a capacity has to hold."""
        bucket_off = np.ascontiguousarray(bucket_off, dtype=np.uint64)
        counts = np.zeros(4, np.uint64)
        self.junction_counts = counts
        check(load().umi_junction_matrix_device(self._h, d_read_ref or None, d_read_pos or None, d_cigar or None,
                                                d_cigar_off or None, d_read_entry or None, n_reads, d_kept or None,
                                                d_root or None, ptr(bucket_off, C.c_uint64), len(bucket_off) - 1, d_col or None,
                                                n_cols, int(capacity), d_jn_ref or None, d_jn_start or None, d_jn_end or None,
                                                d_out_jn or None, d_out_col or None, d_out_molecules or None,
                                                d_out_reads or None, ptr(counts, C.c_uint64), stream or None))
        return counts

    def saturation_curve(self, read_entry, kept, root, bucket_off, row, col, n_rows, n_cols, n_levels=10, seed=0, cell_mask=None):
        """Sequencing saturation and medians per cell as a function of depth (umi_saturation_curve; the rule is in
        include/umihip.h): velocity_matrix's arguments without the classes, n_levels depths, the seed of the reads'
        hash, cell_mask uint8 [n_cols] or None (every column with a molecule is selected).  Returns uint64
        [n_levels, 8], row j the sample of (j + 1) / n_levels of the reads, its columns SATURATION_COLUMNS.  The
        collapse is the full-depth one; nothing is collapsed again per depth."""
        read_entry = np.ascontiguousarray(read_entry, dtype=np.uint32).reshape(-1)
        kept = np.ascontiguousarray(kept, dtype=np.uint8)
        root = np.ascontiguousarray(root, dtype=np.uint32)
        bucket_off = np.ascontiguousarray(bucket_off, dtype=np.uint64)
        row = np.ascontiguousarray(row, dtype=np.uint32)
        col = np.ascontiguousarray(col, dtype=np.uint32)
        nb = len(bucket_off) - 1
        if nb < 0 or len(row) != nb or len(col) != nb:
            raise ValueError("row / col want one element per bucket")
        if len(kept) != len(root) or (nb and int(bucket_off.max()) > len(kept)):
            raise ValueError("kept / root lengths differ, or bucket_off runs past them")
        if cell_mask is not None:
            cell_mask = np.ascontiguousarray(cell_mask, dtype=np.uint8).reshape(-1)
            if len(cell_mask) != n_cols:
                raise ValueError("cell_mask wants one element per column")
        curve = np.zeros((max(1, min(int(n_levels), 32)), 8), np.uint64)
        check(load().umi_saturation_curve(self._h, ptr(read_entry, C.c_uint32), len(read_entry), ptr(kept, C.c_uint8),
                                          ptr(root, C.c_uint32), ptr(bucket_off, C.c_uint64), nb, ptr(row, C.c_uint32),
                                          ptr(col, C.c_uint32), n_rows, n_cols, int(seed), int(n_levels),
                                          None if cell_mask is None else ptr(cell_mask, C.c_uint8), ptr(curve, C.c_uint64)))
        return curve

    def saturation_curve_device(self, d_read_entry, n_reads, d_kept, d_root, bucket_off, d_row, d_col, n_rows, n_cols,
                                n_levels=10, seed=0, d_cell_mask=0, stream=0):
        """The same on raw device pointers (umi_saturation_curve_device; bucket_off stays on the host, and the curve
        comes back in host memory): returns uint64 [n_levels, 8]."""
        bucket_off = np.ascontiguousarray(bucket_off, dtype=np.uint64)
        curve = np.zeros((max(1, min(int(n_levels), 32)), 8), np.uint64)
        check(load().umi_saturation_curve_device(self._h, d_read_entry or None, n_reads, d_kept or None, d_root or None,
                                                 ptr(bucket_off, C.c_uint64), len(bucket_off) - 1, d_row or None, d_col or None,
                                                 n_rows, n_cols, int(seed), int(n_levels), d_cell_mask or None,
                                                 ptr(curve, C.c_uint64), stream or None))
        return curve

    def count_matrix(self, kept, freq, bucket_off, row, col, n_rows, n_cols):
        """Molecules and reads per (column, row) pair (umi_count_matrix): kept uint8 [N] and freq int32 [N] of a
        batched call, bucket_off uint64 [n_buckets + 1], row / col uint32 [n_buckets] the row (gene) and column
        (cell) of every bucket.  Returns (out_row, out_col, molecules uint32, reads uint64), one element per
        distinct pair among the non-empty buckets, sorted by column, then row."""
        kept = np.ascontiguousarray(kept, dtype=np.uint8)
        freq = np.ascontiguousarray(freq, dtype=np.int32)
        bucket_off = np.ascontiguousarray(bucket_off, dtype=np.uint64)
        row = np.ascontiguousarray(row, dtype=np.uint32)
        col = np.ascontiguousarray(col, dtype=np.uint32)
        nb = len(bucket_off) - 1
        if nb < 0 or len(row) != nb or len(col) != nb:
            raise ValueError("row / col want one element per bucket")
        if len(kept) != len(freq) or (nb and int(bucket_off.max()) > len(kept)):
            raise ValueError("kept / freq lengths differ, or bucket_off runs past them")
        m = max(1, nb)
        o_row, o_col, o_mol = (np.zeros(m, np.uint32) for _ in range(3))
        o_reads = np.zeros(m, np.uint64)
        nnz = C.c_uint64(0)
        check(load().umi_count_matrix(self._h, ptr(kept, C.c_uint8), ptr(freq, C.c_int32), ptr(bucket_off, C.c_uint64), nb,
                                      ptr(row, C.c_uint32), ptr(col, C.c_uint32), n_rows, n_cols, ptr(o_row, C.c_uint32),
                                      ptr(o_col, C.c_uint32), ptr(o_mol, C.c_uint32), ptr(o_reads, C.c_uint64),
                                      C.byref(nnz)))
        z = int(nnz.value)
        return o_row[:z], o_col[:z], o_mol[:z], o_reads[:z]

    def count_matrix_device(self, d_kept, d_freq, bucket_off, d_row, d_col, n_rows, n_cols, d_out_row, d_out_col,
                            d_out_molecules, d_out_reads, stream=0):
        """The same on raw device pointers (umi_count_matrix_device; bucket_off stays on the host): fills the
        four output arrays (room for n_buckets elements each) and returns nnz."""
        bucket_off = np.ascontiguousarray(bucket_off, dtype=np.uint64)
        nnz = C.c_uint64(0)
        check(load().umi_count_matrix_device(self._h, d_kept or None, d_freq or None, ptr(bucket_off, C.c_uint64),
                                             len(bucket_off) - 1, d_row or None, d_col or None, n_rows, n_cols,
                                             d_out_row or None, d_out_col or None, d_out_molecules or None,
                                             d_out_reads or None, C.byref(nnz), stream or None))
        return int(nnz.value)

    def filter_multigene(self, keys, freq, kept, root, bucket_off, group, n_groups, umi_len, n_words=1, want_freq=True):
        """UMIs a group shows in several buckets (umi_filter_multigene): keys uint64 [N * n_words], freq int32 [N], kept
        uint8 [N] and root uint32 [N] of a batched call, bucket_off uint64 [n_buckets + 1], group uint32 [n_buckets]
        the group (cell) of every bucket.  Among the kept entries of one group with one UMI only the one with
        strictly the most reads survives.  Returns (kept_out uint8 [N], freq_out int32 [N] or None, dict of
        runs, removed and removed_reads)."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1)
        freq = np.ascontiguousarray(freq, dtype=np.int32)
        kept = np.ascontiguousarray(kept, dtype=np.uint8)
        root = np.ascontiguousarray(root, dtype=np.uint32)
        bucket_off = np.ascontiguousarray(bucket_off, dtype=np.uint64)
        group = np.ascontiguousarray(group, dtype=np.uint32)
        n, nb = len(freq), len(bucket_off) - 1
        if nb < 0 or len(group) != nb:
            raise ValueError("group wants one element per bucket")
        if len(kept) != n or len(root) != n or len(keys) != n * n_words or (nb and int(bucket_off.max()) > n):
            raise ValueError("keys / freq / kept / root lengths differ, or bucket_off runs past them")
        kept_out = np.zeros(n, np.uint8)
        freq_out = np.zeros(n, np.int32) if want_freq else None
        counts = np.zeros(3, np.uint64)
        check(load().umi_filter_multigene(self._h, ptr(keys, C.c_uint64), n_words, umi_len, ptr(freq, C.c_int32),
                                          ptr(kept, C.c_uint8), ptr(root, C.c_uint32), ptr(bucket_off, C.c_uint64), nb,
                                          ptr(group, C.c_uint32), n_groups, ptr(kept_out, C.c_uint8),
                                          ptr(freq_out, C.c_int32), ptr(counts, C.c_uint64)))
        return kept_out, freq_out, self._multigene_counts(counts)

    @staticmethod
    def _multigene_counts(counts):
        return {"runs": int(counts[0]), "removed": int(counts[1]), "removed_reads": int(counts[2])}

    def filter_multigene_device(self, d_keys, d_freq, d_kept, d_root, bucket_off, d_group, n_groups, umi_len, d_kept_out,
                                d_freq_out=0, n_words=1, stream=0):
        """The same on raw device pointers (umi_filter_multigene_device; bucket_off stays on the host): fills
        d_kept_out and, where given, d_freq_out (N elements each) and returns the dict of counts."""
        bucket_off = np.ascontiguousarray(bucket_off, dtype=np.uint64)
        counts = np.zeros(3, np.uint64)
        check(load().umi_filter_multigene_device(self._h, d_keys or None, n_words, umi_len, d_freq or None, d_kept or None,
                                                 d_root or None, ptr(bucket_off, C.c_uint64), len(bucket_off) - 1,
                                                 d_group or None, n_groups, d_kept_out or None, d_freq_out or None,
                                                 ptr(counts, C.c_uint64), stream or None))
        return self._multigene_counts(counts)

    CELLS_COUNTS = ("candidates", "called", "threshold", "knee", "molecules_in_cells", "reads_in_cells", "molecules", "reads",
                    "median_molecules", "median_genes")

    def call_cells(self, row, col, molecules, reads, n_rows, n_cols, rule=UMI_CELLS_CR22, expect_cells=3000,
                   percentile_permille=990, max_min_ratio=10, min_molecules=1):
        """Which columns of a count matrix are cells (umi_call_cells): the triplets row / col / molecules uint32 [nnz]
        and reads uint64 [nnz] as count_matrix returns them, sorted by column, then row.  Returns (dict of the
        per-column arrays cell_molecules, cell_reads uint64, cell_genes uint32, called uint8 and new_col uint32
        [n_cols], the filtered triplets (row, col, molecules, reads) of the called columns, dict of the counts
        CELLS_COUNTS)."""
        row = np.ascontiguousarray(row, dtype=np.uint32)
        col = np.ascontiguousarray(col, dtype=np.uint32)
        molecules = np.ascontiguousarray(molecules, dtype=np.uint32)
        reads = np.ascontiguousarray(reads, dtype=np.uint64)
        nnz = len(row)
        if len(col) != nnz or len(molecules) != nnz or len(reads) != nnz:
            raise ValueError("row / col / molecules / reads lengths differ")
        per = {"cell_molecules": np.zeros(n_cols, np.uint64), "cell_reads": np.zeros(n_cols, np.uint64),
               "cell_genes": np.zeros(n_cols, np.uint32), "called": np.zeros(n_cols, np.uint8),
               "new_col": np.zeros(n_cols, np.uint32)}
        m = max(1, nnz)
        o_row, o_col, o_mol = (np.zeros(m, np.uint32) for _ in range(3))
        o_reads = np.zeros(m, np.uint64)
        nnz_out = C.c_uint64(0)
        counts = np.zeros(10, np.uint64)
        check(load().umi_call_cells(self._h, ptr(row, C.c_uint32), ptr(col, C.c_uint32), ptr(molecules, C.c_uint32),
                                    ptr(reads, C.c_uint64), nnz, n_rows, n_cols, rule, expect_cells, percentile_permille,
                                    max_min_ratio, min_molecules, ptr(per["cell_molecules"], C.c_uint64),
                                    ptr(per["cell_reads"], C.c_uint64), ptr(per["cell_genes"], C.c_uint32),
                                    ptr(per["called"], C.c_uint8), ptr(per["new_col"], C.c_uint32), ptr(o_row, C.c_uint32),
                                    ptr(o_col, C.c_uint32), ptr(o_mol, C.c_uint32), ptr(o_reads, C.c_uint64),
                                    C.byref(nnz_out), ptr(counts, C.c_uint64)))
        z = int(nnz_out.value)
        return per, (o_row[:z], o_col[:z], o_mol[:z], o_reads[:z]), self._cells_counts(counts)

    @classmethod
    def _cells_counts(cls, counts):
        return {name: int(v) for name, v in zip(cls.CELLS_COUNTS, counts)}

    def call_cells_device(self, d_row, d_col, d_molecules, d_reads, nnz, n_rows, n_cols, d_cell_molecules, d_cell_reads,
                          d_cell_genes, d_called, d_new_col, d_out_row, d_out_col, d_out_molecules, d_out_reads,
                          rule=UMI_CELLS_CR22, expect_cells=3000, percentile_permille=990, max_min_ratio=10, min_molecules=1,
                          stream=0):
        """The same on raw device pointers (umi_call_cells_device): fills the five per-column arrays (n_cols
        elements each) and the filtered triplets (room for nnz each); returns (nnz_out, dict of the counts)."""
        nnz_out = C.c_uint64(0)
        counts = np.zeros(10, np.uint64)
        check(load().umi_call_cells_device(self._h, d_row or None, d_col or None, d_molecules or None, d_reads or None, nnz,
                                           n_rows, n_cols, rule, expect_cells, percentile_permille, max_min_ratio,
                                           min_molecules, d_cell_molecules or None, d_cell_reads or None,
                                           d_cell_genes or None, d_called or None, d_new_col or None, d_out_row or None,
                                           d_out_col or None, d_out_molecules or None, d_out_reads or None,
                                           C.byref(nnz_out), ptr(counts, C.c_uint64), stream or None))
        return int(nnz_out.value), self._cells_counts(counts)

    def dedup_stats(self, keys, freq, kept, root, bucket_off, umi_len, n_words=1, seed=0, hist_bins=65536, per_umi=True):
        """What a batched call did, as tables (umi_dedup_stats): keys uint64 [N * n_words], freq int32 [N], kept uint8
        [N] and root uint32 [N] of the call, bucket_off uint64 [n_buckets + 1].  Returns a dict: count_pre / count_post
        uint64 [hist_bins] (family sizes before and after), dist uint64 [4, umi_len + 2] (rows pre, pre-null, post,
        post-null; columns the bins 0..umi_len, then "single") and, with per_umi, umi_entry / times_pre / reads_pre /
        times_post / reads_post, one element per distinct key in ascending key order."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1)
        freq = np.ascontiguousarray(freq, dtype=np.int32)
        kept = np.ascontiguousarray(kept, dtype=np.uint8)
        root = np.ascontiguousarray(root, dtype=np.uint32)
        bucket_off = np.ascontiguousarray(bucket_off, dtype=np.uint64)
        n, nb = len(freq), len(bucket_off) - 1
        if nb < 0 or len(kept) != n or len(root) != n or len(keys) != n * n_words or (nb and int(bucket_off.max()) > n):
            raise ValueError("keys / freq / kept / root lengths differ, or bucket_off runs past them")
        count_pre = np.zeros(max(1, hist_bins), np.uint64)
        count_post = np.zeros(max(1, hist_bins), np.uint64)
        dist = np.zeros((4, max(1, umi_len) + 2), np.uint64)
        out = {"count_pre": count_pre, "count_post": count_post, "dist": dist}
        m = max(1, n)
        tab = {}
        if per_umi:
            tab = {"umi_entry": np.zeros(m, np.uint32), "times_pre": np.zeros(m, np.uint32), "reads_pre": np.zeros(m, np.uint64),
                   "times_post": np.zeros(m, np.uint32), "reads_post": np.zeros(m, np.uint64)}
        rows = C.c_uint64(0)
        check(load().umi_dedup_stats(self._h, ptr(keys, C.c_uint64), n_words, ptr(freq, C.c_int32), ptr(kept, C.c_uint8),
                                     ptr(root, C.c_uint32), ptr(bucket_off, C.c_uint64), nb, umi_len, seed, hist_bins,
                                     ptr(count_pre, C.c_uint64), ptr(count_post, C.c_uint64), ptr(dist, C.c_uint64),
                                     ptr(tab.get("umi_entry"), C.c_uint32), ptr(tab.get("times_pre"), C.c_uint32),
                                     ptr(tab.get("reads_pre"), C.c_uint64), ptr(tab.get("times_post"), C.c_uint32),
                                     ptr(tab.get("reads_post"), C.c_uint64), C.byref(rows) if per_umi else None))
        for name, a in tab.items():
            out[name] = a[:int(rows.value)]
        return out

    def dedup_stats_device(self, d_keys, d_freq, d_kept, d_root, bucket_off, umi_len, d_count_pre, d_count_post, d_dist,
                           n_words=1, seed=0, hist_bins=65536, d_umi_entry=0, d_times_pre=0, d_reads_pre=0, d_times_post=0,
                           d_reads_post=0, stream=0):
        """The same on raw device pointers (umi_dedup_stats_device; bucket_off stays on the host): fills the three
        tables and, where its five arrays are given (room for N elements each), the per-UMI table; returns its rows
        (0 without it)."""
        bucket_off = np.ascontiguousarray(bucket_off, dtype=np.uint64)
        rows = C.c_uint64(0)
        check(load().umi_dedup_stats_device(self._h, d_keys or None, n_words, d_freq or None, d_kept or None, d_root or None,
                                            ptr(bucket_off, C.c_uint64), len(bucket_off) - 1, umi_len, seed, hist_bins,
                                            d_count_pre or None, d_count_post or None, d_dist or None, d_umi_entry or None,
                                            d_times_pre or None, d_reads_pre or None, d_times_post or None,
                                            d_reads_post or None, C.byref(rows), stream or None))
        return int(rows.value)

    def stage_reads(self, align_key, umi_bytes, score, umi_len, merge=1, align_key_bits=64):
        """Read staging on the device (host arrays in and out): reads in file order ->
        dict(keys, nmask, freq, rep, bucket_off) in canonical order, the batched path's input
        (src/deduplicate_sam.rs:148-176 + the rank order of src/algo/directional.rs:67-72)."""
        align_key = np.ascontiguousarray(align_key, dtype=np.uint64)
        umi_bytes = np.ascontiguousarray(umi_bytes, dtype=np.uint8)
        sc = None if score is None else np.ascontiguousarray(score, dtype=np.int32)
        n = len(align_key)
        assert len(umi_bytes) == n * umi_len
        m = max(1, n)
        keys, nm, rep = (np.zeros(m, np.uint64) for _ in range(3))
        freq = np.zeros(m, np.int32)
        boff = np.zeros(m + 1, np.uint64)
        ne, nb = C.c_uint64(0), C.c_uint64(0)
        check(load().umi_stage_reads(self._h, ptr(align_key, C.c_uint64), align_key_bits,
                                        ptr(umi_bytes, C.c_uint8), ptr(sc, C.c_int32), n, umi_len, merge,
                                        ptr(keys, C.c_uint64), ptr(nm, C.c_uint64), ptr(freq, C.c_int32),
                                        ptr(rep, C.c_uint64), ptr(boff, C.c_uint64), C.byref(ne), C.byref(nb)))
        e, b = int(ne.value), int(nb.value)
        return dict(keys=keys[:e], nmask=nm[:e], freq=freq[:e], rep=rep[:e], bucket_off=boff[:b + 1])

    def stage_reads_wide(self, align_key, umi_bytes, score, umi_len, merge=1, align_key_bits=64):
        """stage_reads for UMIs of any length up to 85 bases: keys / nmask come back as uint64
        [n_entries, n_words] (the input of dedup_batch_wide; one column for umi_len <= 21)."""
        align_key = np.ascontiguousarray(align_key, dtype=np.uint64)
        umi_bytes = np.ascontiguousarray(umi_bytes, dtype=np.uint8)
        sc = None if score is None else np.ascontiguousarray(score, dtype=np.int32)
        n, w = len(align_key), (3 * umi_len + 63) // 64
        assert len(umi_bytes) == n * umi_len
        m = max(1, n)
        keys, nm = np.zeros((m, w), np.uint64), np.zeros((m, w), np.uint64)
        rep, freq, boff = np.zeros(m, np.uint64), np.zeros(m, np.int32), np.zeros(m + 1, np.uint64)
        ne, nb = C.c_uint64(0), C.c_uint64(0)
        check(load().umi_stage_reads_wide(self._h, ptr(align_key, C.c_uint64), align_key_bits, ptr(umi_bytes, C.c_uint8),
                                          ptr(sc, C.c_int32), n, umi_len, w, merge, ptr(keys, C.c_uint64),
                                          ptr(nm, C.c_uint64), ptr(freq, C.c_int32), ptr(rep, C.c_uint64),
                                          ptr(boff, C.c_uint64), C.byref(ne), C.byref(nb)))
        e, b = int(ne.value), int(nb.value)
        return dict(keys=keys[:e], nmask=nm[:e], freq=freq[:e], rep=rep[:e], bucket_off=boff[:b + 1])

    def stage_reads_grouped(self, align_key, group_key, umi_bytes, score, umi_len, merge=1, align_key_bits=64,
                            group_key_bits=64):
        """stage_reads with a second per-read key (umi_stage_reads_grouped): positions are
        (align_key, group_key) pairs, e.g. (alignment, cell barcode id); group_key_bits=0 is stage_reads."""
        return self._stage_grouped(align_key, group_key, umi_bytes, score, umi_len, merge, align_key_bits,
                                   group_key_bits, wide=False)

    def stage_reads_grouped_wide(self, align_key, group_key, umi_bytes, score, umi_len, merge=1, align_key_bits=64,
                                 group_key_bits=64):
        """stage_reads_wide with a second per-read key (umi_stage_reads_grouped_wide): keys / nmask
        come back as uint64 [n_entries, n_words]."""
        return self._stage_grouped(align_key, group_key, umi_bytes, score, umi_len, merge, align_key_bits,
                                   group_key_bits, wide=True)

    def _stage_grouped(self, align_key, group_key, umi_bytes, score, umi_len, merge, align_key_bits, group_key_bits,
                       wide):
        align_key = np.ascontiguousarray(align_key, dtype=np.uint64)
        group_key = np.ascontiguousarray(group_key, dtype=np.uint64)
        umi_bytes = np.ascontiguousarray(umi_bytes, dtype=np.uint8)
        sc = None if score is None else np.ascontiguousarray(score, dtype=np.int32)
        n, w = len(align_key), (3 * umi_len + 63) // 64
        assert len(group_key) == n and len(umi_bytes) == n * umi_len
        m = max(1, n)
        shape = (m, w) if wide else m
        keys, nm = np.zeros(shape, np.uint64), np.zeros(shape, np.uint64)
        rep, freq, boff = np.zeros(m, np.uint64), np.zeros(m, np.int32), np.zeros(m + 1, np.uint64)
        ne, nb = C.c_uint64(0), C.c_uint64(0)
        head = (self._h, ptr(align_key, C.c_uint64), align_key_bits, ptr(group_key, C.c_uint64), group_key_bits,
                ptr(umi_bytes, C.c_uint8), ptr(sc, C.c_int32), n, umi_len)
        tail = (merge, ptr(keys, C.c_uint64), ptr(nm, C.c_uint64), ptr(freq, C.c_int32), ptr(rep, C.c_uint64),
                ptr(boff, C.c_uint64), C.byref(ne), C.byref(nb))
        if wide:
            check(load().umi_stage_reads_grouped_wide(*head, w, *tail))
        else:
            check(load().umi_stage_reads_grouped(*head, *tail))
        e, b = int(ne.value), int(nb.value)
        return dict(keys=keys[:e], nmask=nm[:e], freq=freq[:e], rep=rep[:e], bucket_off=boff[:b + 1])

    def stage_reads_grouped_device(self, d_align_key, d_group_key, d_umi, d_score, n_reads, umi_len, d_keys, d_nmask,
                                   d_freq, d_rep, d_bucket_off, merge=1, align_key_bits=64, group_key_bits=64, stream=0):
        """umi_stage_reads_grouped_device (raw device pointers); returns (n_entries, n_buckets)."""
        ne, nb = C.c_uint64(0), C.c_uint64(0)
        check(load().umi_stage_reads_grouped_device(self._h, d_align_key, align_key_bits, d_group_key or None,
                                                    group_key_bits, d_umi, d_score or None, n_reads, umi_len, merge,
                                                    d_keys, d_nmask or None, d_freq, d_rep, d_bucket_off, C.byref(ne),
                                                    C.byref(nb), stream or None))
        return int(ne.value), int(nb.value)

    def stage_reads_grouped_wide_device(self, d_align_key, d_group_key, d_umi, d_score, n_reads, umi_len, d_keys,
                                        d_nmask, d_freq, d_rep, d_bucket_off, merge=1, align_key_bits=64,
                                        group_key_bits=64, stream=0):
        """umi_stage_reads_grouped_wide_device (raw device pointers): UMIs of up to 85 bases, keys / nmask
        ceil(3 * umi_len / 64) words per entry; group_key_bits=0 (d_group_key may then be 0) is the plain
        umi_stage_reads_wide_device, as in the C ABI.  Returns (n_entries, n_buckets)."""
        ne, nb = C.c_uint64(0), C.c_uint64(0)
        check(load().umi_stage_reads_grouped_wide_device(self._h, d_align_key, align_key_bits, d_group_key or None,
                                                         group_key_bits, d_umi, d_score or None, n_reads, umi_len,
                                                         (3 * umi_len + 63) // 64, merge, d_keys, d_nmask or None,
                                                         d_freq, d_rep, d_bucket_off, C.byref(ne), C.byref(nb),
                                                         stream or None))
        return int(ne.value), int(nb.value)

    def stage_reads_device(self, d_align_key, d_umi, d_score, n_reads, umi_len, d_keys, d_nmask, d_freq,
                           d_rep, d_bucket_off, merge=1, align_key_bits=64, stream=0):
        """The same with everything in device memory (raw pointers); returns (n_entries, n_buckets)."""
        ne, nb = C.c_uint64(0), C.c_uint64(0)
        check(load().umi_stage_reads_device(self._h, d_align_key, align_key_bits, d_umi, d_score or None,
                                               n_reads, umi_len, merge, d_keys, d_nmask or None, d_freq, d_rep,
                                               d_bucket_off, C.byref(ne), C.byref(nb), stream or None))
        return int(ne.value), int(nb.value)

    def dedup_batch_device(self, d_keys, d_nmask, d_freq, bucket_off, umi_len, d_kept, d_root=0,
                           k=1, percentage=0.5, algo=UMI_ALGO_DIRECTIONAL, adj_max_freq=0,
                           stream=0, d_bucket_off=0):
        """Device-pointer batched call (integers = device addresses, e.g. tensor.data_ptr()).
        d_bucket_off: device copy of bucket_off, if the caller keeps one (no upload inside)."""
        bucket_off = np.ascontiguousarray(bucket_off, dtype=np.uint64)
        st = Stats()
        check(load().umi_dedup_batch_device_table(self._h, d_keys, d_nmask or None, d_freq,
                                                  ptr(bucket_off, C.c_uint64), d_bucket_off or None,
                                                  len(bucket_off) - 1, umi_len, k, percentage, algo,
                                                  adj_max_freq, d_kept, d_root or None, stream or None,
                                                  C.byref(st)))
        return st.as_dict()

    def dedup_batch_edit_device(self, d_keys, d_nmask, d_freq, bucket_off, umi_len, d_kept, d_root=0,
                                k=1, percentage=0.5, algo=UMI_ALGO_DIRECTIONAL, adj_max_freq=0, stream=0):
        """umi_dedup_batch_edit_device: dedup_batch_device by Levenshtein distance."""
        bucket_off = np.ascontiguousarray(bucket_off, dtype=np.uint64)
        st = Stats()
        check(load().umi_dedup_batch_edit_device(self._h, d_keys, d_nmask or None, d_freq,
                                                 ptr(bucket_off, C.c_uint64), len(bucket_off) - 1, umi_len, k,
                                                 percentage, algo, adj_max_freq, d_kept, d_root or None,
                                                 stream or None, C.byref(st)))
        return st.as_dict()

    def dedup_batch_cr_device(self, d_keys, d_nmask, d_freq, bucket_off, umi_len, d_kept, d_root=0, d_target=0,
                              stream=0):
        """umi_dedup_batch_cr_device: dedup_batch_cr on device pointers (d_root and d_target may be 0)."""
        bucket_off = np.ascontiguousarray(bucket_off, dtype=np.uint64)
        st = Stats()
        check(load().umi_dedup_batch_cr_device(self._h, d_keys, d_nmask or None, d_freq, ptr(bucket_off, C.c_uint64),
                                               len(bucket_off) - 1, umi_len, d_kept, d_root or None, d_target or None,
                                               stream or None, C.byref(st)))
        return st.as_dict()

    def dedup_batch_device_begin(self, d_keys, d_nmask, d_freq, bucket_off, umi_len, d_kept, d_root=0,
                                 k=1, percentage=0.5, algo=UMI_ALGO_DIRECTIONAL, adj_max_freq=0,
                                 stream=0, d_bucket_off=0):
        """umi_dedup_batch_device_begin: the device-pointer call enqueued on `stream`; where every position is
        the fused kernel's it returns without waiting (d_kept / d_root final in stream order), else it
        runs to its end.  dedup_batch_end() waits and returns the stats."""
        bucket_off = np.ascontiguousarray(bucket_off, dtype=np.uint64)
        check(load().umi_dedup_batch_device_begin(self._h, d_keys, d_nmask or None, d_freq,
                                                  ptr(bucket_off, C.c_uint64), d_bucket_off or None,
                                                  len(bucket_off) - 1, umi_len, k, percentage, algo,
                                                  adj_max_freq, d_kept, d_root or None, stream or None))

    def dedup_batch_end(self):
        st = Stats()
        check(load().umi_dedup_batch_end(self._h, C.byref(st)))
        return st.as_dict()

    def dedup_batch_device_multi(self, shards, umi_len, slice_bytes, k=1, percentage=0.5, algo=UMI_ALGO_DIRECTIONAL,
                                 adj_max_freq=0, gather=True):
        """umi_dedup_batch_device_multi on a multi-device context: shards = one dict per device with the
        device addresses d_keys, d_freq, d_kept (and optionally d_nmask, d_root), the host array
        bucket_off, and d_bits_all (n_devices * slice_bytes bytes on that device) for the RCCL
        all-gather of the packed kept masks.  Returns the merged stats."""
        nd = len(shards)
        boffs = [np.ascontiguousarray(sh["bucket_off"], dtype=np.uint64) for sh in shards]

        def ptrs(name, required=True):
            vals = [sh.get(name) or None for sh in shards]
            if not required and all(v is None for v in vals):
                return None
            return (C.c_void_p * nd)(*vals)
        st = Stats()
        off_arr = (_lib._u64p * nd)(*[ptr(b, C.c_uint64) for b in boffs])
        nb_arr = (C.c_uint64 * nd)(*[len(b) - 1 for b in boffs])
        check(load().umi_dedup_batch_device_multi(self._h, ptrs("d_keys"), ptrs("d_nmask", False), ptrs("d_freq"), off_arr,
                                                  nb_arr, umi_len, k, percentage, algo, adj_max_freq, ptrs("d_kept"),
                                                  ptrs("d_root", False), ptrs("d_bits_all") if gather else None,
                                                  slice_bytes, C.byref(st)))
        return st.as_dict()

    def dedup_batch_wide_device(self, d_keys, d_nmask, n_words, d_freq, bucket_off, umi_len, d_kept, d_root=0, k=1,
                                percentage=0.5, algo=UMI_ALGO_DIRECTIONAL, adj_max_freq=0, stream=0):
        """Device-pointer batched call for keys of n_words words per entry (umi_len > 21)."""
        bucket_off = np.ascontiguousarray(bucket_off, dtype=np.uint64)
        st = Stats()
        check(load().umi_dedup_batch_wide_device(self._h, d_keys, d_nmask or None, n_words, d_freq, ptr(bucket_off, C.c_uint64),
                                                 len(bucket_off) - 1, umi_len, k, percentage, algo, adj_max_freq, d_kept,
                                                 d_root or None, stream or None, C.byref(st)))
        return st.as_dict()

    def pack_mask_device(self, d_kept, n, d_bits, stream=0):
        """kept bytes -> bits on the device (umi_pack_mask_device), enqueued on `stream`."""
        check(load().umi_pack_mask_device(self._h, d_kept, n, d_bits, stream or None))

    def pairs_partial_device(self, d_keys, d_nmask, d_freq, bucket_off, umi_len, part, n_parts,
                             d_edges, edge_capacity, k=1, percentage=0.5,
                             algo=UMI_ALGO_DIRECTIONAL, adj_max_freq=0, stream=0):
        """This rank's share (every n_parts-th tile task) of the permitted-edge list, written
        to the caller's device buffer d_edges (uint64 entries).  Returns (n_edges, stats);
        raises UmiHipError(UMI_ERR_NOMEM) if edge_capacity is too small (n_edges in the text)."""
        bucket_off = np.ascontiguousarray(bucket_off, dtype=np.uint64)
        st = Stats()
        n_edges = C.c_uint64(0)
        check(load().umi_pairs_partial_device(self._h, d_keys, d_nmask or None, d_freq,
                                              ptr(bucket_off, C.c_uint64), len(bucket_off) - 1,
                                              umi_len, k, percentage, algo, adj_max_freq, part,
                                              n_parts, d_edges, edge_capacity, C.byref(n_edges),
                                              stream or None, C.byref(st)))
        return int(n_edges.value), st.as_dict()

    def collapse_edges_device(self, n, d_edges, n_edges, d_kept, d_root=0,
                              algo=UMI_ALGO_DIRECTIONAL, stream=0):
        """Collapse of a gathered edge list over n entries; fills d_kept / d_root."""
        st = Stats()
        check(load().umi_collapse_edges_device(self._h, n, d_edges or None, n_edges, algo, d_kept,
                                               d_root or None, stream or None, C.byref(st)))
        return st.as_dict()


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


class HipNaive:
    """DataStruct (src/data/mod.rs:11-17) with Naive's semantics (src/data/naive.rs),
    neighbour lists built on the GPU at construction.  UMIs are ASCII strings here
    (the reference's &BitSet keys); insertion order of `umi_freq` is kept."""

    def __init__(self):  # Default
        self._h = None
        self._index = {}
        self._umis = []

    @classmethod
    def new(cls, umi_freq, umi_length, max_edits, ctx=None):
        """DataStruct::new(umi_freq: HashMap<&BitSet,i32>, umi_length, max_edits)"""
        self = cls()
        ctx = ctx or default_context()
        self._ctx = ctx
        self._umis = list(umi_freq.keys())
        self._index = {u: i for i, u in enumerate(self._umis)}
        freq = np.array([umi_freq[u] for u in self._umis], dtype=np.int32)
        self._n = len(self._umis)
        h = C.c_void_p()
        if umi_length > _lib.UMI_MAX_UMI_LEN:  # keys of several words (bitset.rs:17-27)
            words = (3 * umi_length + 63) // 64
            keys, nmask = to_bitset_wide([u if isinstance(u, str) else u.decode() for u in self._umis], umi_length) \
                if self._umis else (np.zeros((0, words), np.uint64), np.zeros((0, words), np.uint64))
            check(load().umi_data_new_wide(ctx._h, ptr(keys, C.c_uint64), ptr(nmask, C.c_uint64) if nmask.any() else None,
                                           words, ptr(freq, C.c_int32), self._n, umi_length, max_edits, C.byref(h)))
            self._h = h
            return self
        keys, nmask = to_bitset(self._umis, umi_length) if self._umis else (
            np.zeros(0, np.uint64), np.zeros(0, np.uint64))
        check(load().umi_data_new(ctx._h, ptr(keys, C.c_uint64),
                                  ptr(nmask, C.c_uint64) if nmask.any() else None,
                                  ptr(freq, C.c_int32), self._n, umi_length, max_edits,
                                  C.byref(h)))
        self._h = h
        return self

    def remove_near(self, umi, k, max_freq):
        """-> set of removed UMIs (HashSet<&BitSet>)"""
        out = np.zeros(max(1, self._n), dtype=np.uint32)
        cnt = C.c_uint32(0)
        check(load().umi_data_remove_near(self._h, self._index[umi], k, max_freq,
                                          ptr(out, C.c_uint32), C.byref(cnt)))
        return {self._umis[i] for i in out[:cnt.value]}

    def contains(self, umi):
        i = self._index.get(umi)
        if i is None:
            return False
        rc = load().umi_data_contains(self._h, i)
        if rc < 0:
            check(rc)
        return rc == 1

    def stats(self):
        return {}

    def __del__(self):
        if getattr(self, "_h", None):
            load().umi_data_free(self._h)
            self._h = None


class ReadFreq:
    """src/utils/read_freq.rs:4-13"""
    __slots__ = ("read", "freq")

    def __init__(self, read, freq):
        self.read, self.freq = read, freq


def _f32_as_i32(x):
    x = np.float32(x)
    if np.isnan(x):
        return 0
    return int(max(-2 ** 31, min(2 ** 31 - 1, int(x))))


class Directional:
    """src/algo/directional.rs:15-91.  apply() follows the reference's control flow
    over any DataStruct (default HipNaive): stable freq-descending sort, root loop,
    neighbour visit (explicit stack instead of the reference's recursion)."""

    def __init__(self, k=1, percentage=0.5, track_cluster=False):
        self.k, self.percentage, self.track_cluster = k, np.float32(percentage), track_cluster

    def _visit_and_remove(self, start_umi, reads, data, cluster):
        stack = [start_umi]
        while stack:
            u = stack.pop()
            f1 = (reads[u].freq + 1 + 2 ** 31) % 2 ** 32 - 2 ** 31  # i32 wrap, as a release build
            threshold = _f32_as_i32(self.percentage * np.float32(f1))
            near = data.remove_near(u, self.k, threshold)
            if cluster is not None:
                cluster.extend(near)
            stack.extend(v for v in near if v != u)

    def apply(self, reads, tracker, umi_length, data_struct=HipNaive):
        """reads: dict umi -> ReadFreq in first-appearance order.  Returns list of reads."""
        data_member = {umi: rf.freq for umi, rf in reads.items()}
        umi_freqs = sorted(reads.items(), key=lambda kv: -kv[1].freq)  # stable
        data = data_struct.new(data_member, umi_length, self.k)
        res = []
        for umi, rf in umi_freqs:
            if data.contains(umi):
                cluster = [] if (self.track_cluster and tracker is not None) else None
                self._visit_and_remove(umi, reads, data, cluster)
                if cluster is not None:
                    tracker[umi] = cluster
                res.append(rf.read)
        return res


class Adjacency:
    """src/algo/adjacency.rs:15-63 (remove_near(umi, k, 0): reference behaviour)."""

    def __init__(self, k=1, percentage=0.5, track_cluster=False, max_freq=0):
        self.k, self.percentage, self.track_cluster = k, percentage, track_cluster
        self.max_freq = max_freq

    def apply(self, reads, tracker, umi_length, data_struct=HipNaive):
        freq = sorted(reads.items(), key=lambda kv: -kv[1].freq)
        m = {umi: rf.freq for umi, rf in reads.items()}
        data = data_struct.new(m, umi_length, self.k)
        res = []
        for umi, rf in freq:
            if data.contains(umi):
                near = data.remove_near(umi, self.k, self.max_freq)
                if tracker is not None:
                    tracker[umi] = sorted(near)
                res.append(rf.read)
        return res


class Cluster:
    """Connected components of "within k" (UMI_ALGO_CLUSTER; umi_tools' `cluster`, UMICollapse's `cc`,
    STARsolo's 1MM_All at k = 1): the root loop of Directional with every neighbour admitted whatever its
    freq -- remove_near(u, k, INT32_MAX), followed transitively -- so a root takes its whole component
    and the survivor is the component's first UMI in rank order.  percentage is accepted and plays no part."""

    def __init__(self, k=1, percentage=0.5, track_cluster=False):
        self.k, self.percentage, self.track_cluster = k, percentage, track_cluster

    def apply(self, reads, tracker, umi_length, data_struct=HipNaive):
        """reads: dict umi -> ReadFreq in first-appearance order.  Returns list of reads."""
        data_member = {umi: rf.freq for umi, rf in reads.items()}
        umi_freqs = sorted(reads.items(), key=lambda kv: -kv[1].freq)  # stable
        data = data_struct.new(data_member, umi_length, self.k)
        res = []
        for umi, rf in umi_freqs:
            if data.contains(umi):
                cluster = [] if (self.track_cluster and tracker is not None) else None
                stack = [umi]
                while stack:
                    u = stack.pop()
                    near = data.remove_near(u, self.k, 2 ** 31 - 1)
                    if cluster is not None:
                        cluster.extend(near)
                    stack.extend(v for v in near if v != u)
                if cluster is not None:
                    tracker[umi] = cluster
                res.append(rf.read)
        return res
