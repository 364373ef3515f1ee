"""Tensor-level wrappers over the C-ABI (whisprrec_amd.abi).

PyTorch-ROCm is used here only as the owner of device memory and of the HIP stream; every computation is a
call into libwhisprrec_hip.so on ``torch.cuda.current_stream()``.  Nothing in this module has a CPU path:
tensors must live on a ROCm device and the library must be built.
"""
import ctypes

import torch

from . import abi


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _addr(struct):
    """address of a ctypes struct / array, or None"""
    return ctypes.addressof(struct) if struct is not None else None


def _event_handles(events, per_step, count, allow_none):
    """the hipEvent_t handles of `per_step * count` ``torch.cuda.Event(enable_timing=True)`` as a c_void_p array for the
    step entries' timing hooks (None: no hooks).  allow_none: single entries may be None."""
    if events is None:
        return None
    if len(events) != per_step * count:
        raise ValueError("%s must hold %d events per step" % ("phase_events" if per_step == 4 else "events", per_step))
    handles = []
    for e in events:
        if e is None and allow_none:
            handles.append(None)
            continue
        if not e.cuda_event:  # torch creates the hipEvent_t lazily on first record
            e.record()
        handles.append(e.cuda_event)
    return (ctypes.c_void_p * len(handles))(*handles)


def _auto_lag(state, plan):
    """max_lag of an optimizer state: its own setting, or (None) MAX_LAG when a row misses more than LAG_MIN_GAP steps between
    two uses on average (rows / batch), else 0 = unbounded"""
    if state.max_lag is None:
        gap = max(state.tabs.U.shape[0], state.tabs.I.shape[0]) / float(max(plan.batch_size, 1))
        return state.MAX_LAG if gap > state.LAG_MIN_GAP else 0
    return state.max_lag


def _req(t, dtype, name, ndim=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if t.device.type != "cuda":
        raise abi.WhisprRecHipError("%s must live on a ROCm device (got %s); there is no CPU fallback" % (name, t.device))
    if t.dtype != dtype:
        raise TypeError("%s must be %s (got %s)" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    if ndim is not None and t.dim() != ndim:
        raise ValueError("%s must have %d dims (got %d)" % (name, ndim, t.dim()))
    return t


def _idx64(t, name):
    """Reference batches are int64 tensors (src/models/BaseModel.py:121)."""
    if t.dtype != torch.int64:
        t = t.to(torch.int64)
    return _req(t.contiguous(), torch.int64, name)


class Workspace:
    """A growable byte buffer handed to the library as caller-owned scratch."""

    def __init__(self, device):
        self.device = device
        self.buf = None

    def get(self, nbytes):
        nbytes = int(nbytes)
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=self.device)
        return self.buf


_WS = {}


def workspace(device, tag):
    """scratch buffer per (device, tag, current stream): two streams never share scratch, whoever created them"""
    sid = torch.cuda.current_stream(device).cuda_stream if torch.device(device).type == "cuda" else 0
    key = (str(device), tag, sid)
    if key not in _WS:
        _WS[key] = Workspace(device)
    return _WS[key]


_SHAPE_WS = {}          # (tag, device, stream, shape) -> slot: nothing is allocated after the first call of a shape


def _shape_workspace(tag, dev, shape, nbytes, err_word=False):
    """the workspace of nbytes(*shape) bytes allocated at the first call of `shape` on this device and stream (the fused losses);
    err_word: a zeroed int32 word is kept beside it -> (workspace, word)"""
    key = (tag, str(dev), torch.cuda.current_stream(dev).cuda_stream, shape)
    slot = _SHAPE_WS.get(key)
    if slot is None:
        slot = torch.empty(nbytes(*shape), dtype=torch.uint8, device=dev)
        if err_word:
            slot = (slot, torch.zeros(1, dtype=torch.int32, device=dev))
        _SHAPE_WS[key] = slot
    return slot


def _release_shape_workspaces(tag):
    for key in [k for k in _SHAPE_WS if k[0] == tag]:
        del _SHAPE_WS[key]


def _loss_slot(loss, dev):
    """the `loss=` argument of the fused losses -> (the (1,) tensor the kernel writes, accumulate into it or overwrite)"""
    if loss is None:
        return torch.empty(1, dtype=torch.float32, device=dev), False
    _req(loss, torch.float32, "loss")
    if loss.numel() != 1:
        raise ValueError("loss must hold one element")
    return loss, True


def _check_tau(tau):
    if not (float(tau) > 0.0):
        raise ValueError("tau must be positive (got %r)" % (tau,))


def side_stream(device):
    """A stream for work that must OVERLAP the step kernels (plan builds, ring transfers).  HIP spreads the streams of
    one priority round-robin over a few hardware queues, and two streams that land on the same queue run one after the
    other (seen in a kernel trace: plan stream and main stream both on queue 4, every plan build waiting for the step
    kernels to drain).  A high-priority stream has its own queue, and the small kernels it carries should not wait behind
    the whole-GPU step kernels anyway."""
    return torch.cuda.Stream(device=device, priority=-1)


def device_info():
    n_cu, wave = ctypes.c_int32(0), ctypes.c_int32(0)
    arch = ctypes.create_string_buffer(64)
    abi.check(abi.lib().wr_device_info(ctypes.addressof(n_cu), ctypes.addressof(wave), ctypes.addressof(arch), 64),
              "wr_device_info")
    return {"n_cu": n_cu.value, "wave_size": wave.value, "arch": arch.value.decode()}


# ----------------------------------------------------------------------------------------------- forward
def bpr_fwd(user_tab, item_tab, u, p, n, scores=True, coef=False):
    """BPRMF.predict forward (reference src/models/general/BPRMF.py:69-80, src/utils/loss.py:37-39).

    Returns dict(loss=0-d tensor, pos_score, neg_score, coef) — the optional entries are None when not asked."""
    L = abi.lib()
    _req(user_tab, torch.float32, "user_tab", 2)
    _req(item_tab, torch.float32, "item_tab", 2)
    u, p, n = _idx64(u, "user_id"), _idx64(p, "pos_item"), _idx64(n, "neg_items")
    B, D = u.numel(), user_tab.shape[1]
    if not (p.numel() == B and n.numel() == B):
        raise ValueError("user_id/pos_item/neg_items must have the same length")
    dev = user_tab.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    pos = torch.empty(B, dtype=torch.float32, device=dev) if scores else None
    neg = torch.empty(B, dtype=torch.float32, device=dev) if scores else None
    cf = torch.empty(B, dtype=torch.float32, device=dev) if coef else None
    nbytes = abi.check_size(L.wr_bpr_fwd_workspace_bytes(B), "wr_bpr_fwd_workspace_bytes")
    ws = workspace(dev, "fwd").get(nbytes)
    abi.check(L.wr_bpr_fwd(_p(user_tab), user_tab.shape[0], _p(item_tab), item_tab.shape[0], D, _p(u), _p(p), _p(n), B,
                           _p(pos), _p(neg), _p(cf), _p(loss), _p(ws), ws.numel(), _stream()), "wr_bpr_fwd")
    return {"loss": loss, "pos_score": pos, "neg_score": neg, "coef": cf}


# ----------------------------------------------------------------------------------------------- plan
_FAST_BACKOFF = {}


class BucketMap:
    """Load-balanced row ranges for the hand-written plan builder on skewed ids (struct wr_bucket_side of
    include/whisprrec_hip.h).  Built once per epoch from the id columns with array operations on the device: the expected
    number of triplets (item occurrences) a row contributes to a batch is its share of the epoch's rows times the batch size
    (+ the uniform negatives for items, reference BaseModel.py:167-177); consecutive rows are grouped until a bucket holds
    the mean load, and a row that holds more than half of it on its own becomes one or more buckets of its own (its
    occurrences split by position in the batch).  The buckets ascend with the rows, so the plan is the one every other
    builder emits.  ``users`` / ``items`` are None when that side needs more than 1024 buckets (then: generic builder)."""

    NOMINAL = 256        # the builder's bucket count (and capacity = 2 x mean + 64) in the regime maps are made for
    SAMPLE = 1 << 21     # rows of the epoch the shares are estimated from

    def __init__(self, u, p, n_users, n_items, batch_size):
        B, n = int(batch_size), u.numel()
        dev = u.device
        self.batch_size = B
        # Row shares from a strided sample of at most SAMPLE rows: the buckets need the heavy rows' shares to a few percent
        # and the light rows' only in sums over whole ranges, and torch.bincount's global atomics on 40 M power-law ids
        # take 18 ms (one hot counter) against <1 ms on the sample.  (Out-of-range ids are the plan's business — flags[0],
        # IndexError at validate(); here they only must not break bincount.)
        step = max(1, n // self.SAMPLE)
        us, ps = u[::step].long().clamp_(0, n_users - 1), p[::step].long().clamp_(0, n_items - 1)
        lam_u = torch.bincount(us, minlength=n_users).double() * (B / us.numel())
        lam_i = torch.bincount(ps, minlength=n_items).double() * (B / ps.numel())
        if n_items > 1:                                      # negatives: uniform over [1, n_items)
            lam_i[1:] += B / (n_items - 1)
        self.users = self._side(lam_u, B / self.NOMINAL, dev)
        self.items = self._side(lam_i, 2 * B / self.NOMINAL, dev)

    @staticmethod
    def _side(lam, mean, dev):
        n_rows = lam.numel()
        # heavy: more than half a bucket's mean load — or so many occurrences per batch that one bin of the bucket sort (bins
        # separate ROWS in an ordinary bucket, at most 256 composites each) could not hold them; heavy rows get position bins
        heavy = lam > min(mean / 2, 96.0)
        w = torch.where(heavy, torch.zeros_like(lam), lam)
        before = torch.cumsum(w, 0) - w                                   # load of the ordinary rows in front of each row
        group = torch.floor(before / mean).long()
        nsub = torch.where(heavy, torch.ceil(lam / mean), torch.zeros_like(lam)).long()
        start = torch.ones(n_rows, dtype=torch.bool, device=dev)
        if n_rows > 1:
            start[1:] = (group[1:] != group[:-1]) | heavy[1:] | heavy[:-1]
        extra = torch.zeros(n_rows, dtype=torch.long, device=dev)        # sub-buckets of the heavy row in front
        if n_rows > 1:
            extra[1:] = torch.clamp(nsub[:-1] - 1, min=0)
        first = torch.cumsum(start.long() + extra, 0) - 1                 # id of the row's (first) bucket
        n_buckets = int(first[-1].item()) + max(int(nsub[-1].item()), 1)
        if n_buckets > 1024 or int(nsub.max().item()) >= 65536:
            return None
        row_bucket = (first | (nsub << 16)).to(torch.int32)
        rows_at = torch.nonzero(start).flatten()                          # first row of every run of rows sharing a bucket
        b_start = torch.zeros(n_buckets, dtype=torch.long, device=dev)
        b_rows = torch.ones(n_buckets, dtype=torch.long, device=dev)
        b_sub = torch.zeros(n_buckets, dtype=torch.long, device=dev)
        ids = first[rows_at]
        b_start[ids] = rows_at
        ends = torch.cat([rows_at[1:], torch.tensor([n_rows], device=dev)])
        b_rows[ids] = ends - rows_at
        hrows = torch.nonzero(heavy).flatten()
        if hrows.numel():
            m = nsub[hrows]
            rep = torch.repeat_interleave(torch.arange(hrows.numel(), device=dev), m)      # one entry per sub-bucket
            q = torch.arange(rep.numel(), device=dev) - torch.repeat_interleave(torch.cumsum(m, 0) - m, m)
            ids_h = first[hrows][rep] + q
            b_start[ids_h] = hrows[rep]
            b_rows[ids_h] = 1
            b_sub[ids_h] = q | (m[rep] << 16)
        arrs = [t.to(torch.int32).contiguous() for t in (row_bucket, b_start, b_rows, b_sub)]
        return {"n_buckets": n_buckets, "arrays": arrs,
                "struct": abi.BucketSide(n_buckets, *[a.data_ptr() for a in arrs])}

    def record_stream(self, stream):
        for side in (self.users, self.items):
            if side is not None:
                for a in side["arrays"]:
                    a.record_stream(stream)


class PlanArena:
    """Pre-sized home of ONE plan's arrays (sorted triplets, occurrence lists, hot-run lists, flags + counts and their
    pinned host mirror), allocated once before a step stream starts.  A BatchPlan built into an arena makes no allocation
    (`torch.empty` of a new size ends in hipMalloc, which stalls the host long enough to drain the queue) and its small
    read-back is an asynchronous copy into pinned memory that is consumed when the plan is first used.  PipelinedSgd
    keeps two arenas and alternates them: chunk c+1 is built while chunk c trains."""

    def __init__(self, device, max_triplets, batch_size, hot=True, overlap_items=0):
        N, B = int(max_triplets), int(batch_size)
        self.device, self.max_triplets, self.batch_size = device, N, B
        self.max_batches = (N + B - 1) // B
        i32 = dict(dtype=torch.int32, device=device)
        self.idx = torch.empty(7 * N, **i32)                       # tu | tp | tn | oc_item (2N) | oc_src (2N)
        n_meta = BatchPlan.meta_len(self.max_batches)
        self.meta = torch.zeros(n_meta, **i32)
        self.meta_host = torch.zeros(n_meta, dtype=torch.int32, pin_memory=True)
        self.meta_np = self.meta_host.numpy()      # the same pinned words as a NumPy view: cheap scalar reads on the step path
        self.views = {}                            # BatchPlan.finish: slices of the words above, by plan length
        self.hot_sides = None
        if hot:
            self.hot_sides = []
            for kind in (0, 1):
                cp, cr = hot_caps(B, kind)
                buf = torch.empty(self.max_batches * (2 * cp + 3 * cr), **i32)
                self.hot_sides.append((buf, cp, cr))
        # overlap marks (wr_bprmf_plan_overlap_marks): per batch a bitmap of the item rows with several occurrences, a
        # bitmask of the deferred run heads and their list
        self.overlap = None
        if overlap_items > 0:
            words = (int(overlap_items) + 31) // 32
            dwords = (B + 31) // 32
            self.overlap = {"words": words, "dwords": dwords, "cap": overlap_def_cap(B),
                            "bitmap": torch.empty(self.max_batches * words, **i32),
                            "tdef": torch.empty(self.max_batches * dwords, **i32),
                            "def_q": torch.empty(self.max_batches * overlap_def_cap(B), **i32)}
        self.free = None      # event on the consuming stream: every step that reads this arena's arrays has run

    def release_after(self, stream):
        """the arena's arrays are read by work queued on `stream` up to here; the next build into it waits for that"""
        self.free = torch.cuda.Event()
        self.free.record(stream)


def hot_caps(batch_size, kind):
    cp, cr = ctypes.c_int64(0), ctypes.c_int64(0)
    abi.lib().wr_bprmf_hot_caps(int(batch_size), kind, ctypes.addressof(cp), ctypes.addressof(cr))
    return cp.value, cr.value


def overlap_def_cap(batch_size):
    """capacity of a batch's list of deferred user runs (overlapped step stream)"""
    return max(256, int(batch_size) // 8)


class BatchPlan:
    """Sorted batches for the fused step (see include/whisprrec_hip.h, "Batch plan").

    ``u, p, n`` are the epoch's triplets in batch order (int64 as in the reference, or int32); batch k is
    ``[k*batch_size, (k+1)*batch_size)``, the last one may be short (no drop_last, BaseRunner.py:201).

    The small device-to-host read-back a plan needs (index-range flag, bucket-overflow flag of the hand-written builder,
    hot-run counts) is either taken at once (default: the constructor returns a finished plan) or, with ``defer=True``,
    queued as an asynchronous copy into pinned memory behind the build and consumed by ``finish()`` — which every consumer
    of the plan's host-side state calls, and which costs nothing once the build has run."""

    META_HEAD = 2

    @staticmethod
    def meta_len(n_batches):
        """[0] index out of range, [1] fast-builder bucket overflow, then per batch the number of hot-run pieces and hot
        runs (items, users: wr_bprmf_plan_hot_runs), then per batch the number of deferred user runs (overlap marks)"""
        return BatchPlan.META_HEAD + 5 * int(n_batches)

    def __init__(self, u, p, n, batch_size, n_users, n_items, keep_orig=False, validate=True, ws_tag="plan", builder="auto",
                 hot=True, bucket_map=None, arena=None, defer=False, overlap=False):
        """builder: "auto" (default) = hand-written bucket/LDS-sort builder when applicable, generic radix-sort builder
        otherwise or when a bucket overflowed (skewed ids) — both emit identical arrays; "fast" / "generic" force one;
        "small" = one workgroup per batch in LDS (batch_size <= 4,096), one launch, same arrays.
        bucket_map: a BucketMap of the epoch these batches come from — load-balanced buckets for the hand-written builder
        (skewed ids); ``fast_overflowed`` tells afterwards whether the hand-written builder was tried and gave up.
        arena: a PlanArena to build into (no allocation); defer: do not wait for the read-back (see finish());
        overlap: also compute the marks of the overlapped step stream (wr_bprmf_plan_overlap_marks; needs an arena created
        with overlap_items) — ``self.overlap`` is then set by finish() when the plan qualifies (no hot rows, lists fit)."""
        if u.dtype not in (torch.int64, torch.int32):
            raise TypeError("indices must be int64 or int32")
        dt = u.dtype
        u, p, n = (_req(t.contiguous(), dt, nm, 1) for t, nm in ((u, "u"), (p, "p"), (n, "n")))
        N = u.numel()
        if not (p.numel() == N and n.numel() == N):
            raise ValueError("u/p/n must have the same length")
        if N == 0:
            raise ValueError("empty epoch")
        dev = u.device
        self.n_triplets, self.batch_size = N, int(batch_size)
        self.n_users, self.n_items = int(n_users), int(n_items)
        self.n_batches = (N + self.batch_size - 1) // self.batch_size
        self._src = (u, p, n)
        self._ws_tag, self._want_hot, self._bucket_map = ws_tag, bool(hot), bucket_map
        self._want_overlap = bool(overlap)
        if overlap and (arena is None or arena.overlap is None or not hot):
            raise ValueError("overlap marks need an arena with overlap_items and the hot-run scan")
        self._stream = torch.cuda.current_stream(dev)
        self.arena = arena
        i32 = dict(dtype=torch.int32, device=dev)
        if arena is not None:
            if arena.batch_size != self.batch_size or N > arena.max_triplets or (hot and arena.hot_sides is None):
                raise ValueError("plan does not fit its arena")
            if arena.free is not None:                       # steps that still read the arena's previous plan
                self._stream.wait_event(arena.free)
                arena.free = None
            a, M = arena.idx, arena.max_triplets
            self.tu, self.tp, self.tn = a[:N], a[M:M + N], a[2 * M:2 * M + N]
            self.oc_item, self.oc_src = a[3 * M:3 * M + 2 * N], a[5 * M:5 * M + 2 * N]
            self._cap_batches = arena.max_batches            # the layout of the counts does not depend on this plan's size
            self.meta = arena.meta
            self.meta.zero_()
            self._pinned = arena.meta_host
            self._unchecked = False
        else:
            self.tu, self.tp, self.tn = torch.empty(N, **i32), torch.empty(N, **i32), torch.empty(N, **i32)
            self.oc_item, self.oc_src = torch.empty(2 * N, **i32), torch.empty(2 * N, **i32)
            self._cap_batches = self.n_batches
            # a single-workgroup plan nobody will ask for its flags (indices range-checked by the caller, no hot-run scan):
            # no flag words to clear — one launch less in a step that builds a plan of its own (LightGCN)
            self._unchecked = builder == "small" and not validate and not hot and not overlap
            self.meta = (torch.empty if self._unchecked else torch.zeros)(self.meta_len(self.n_batches), **i32)
            self._pinned = None
        self.torig = torch.empty(N, **i32) if keep_orig else None
        self.flags = self.meta[:2]
        self.err = self.flags[:1]
        self.hot = None
        self.builder = None
        self.overlap = None
        self.meta_host = None
        self.ready = None
        self.fast_overflowed = False
        self._finished = False
        self._sides = None
        self._tried = None           # "fast" / "fast+map": the hand-written builder ran and its overflow flag is pending
        # "auto": ids skewed enough to overflow a bucket keep doing so chunk after chunk — after an overflow the next 32
        # plans of the same shape go straight to the radix-sort builder instead of paying for a failed attempt each
        self._backoff_key = (str(dev), self.batch_size, self.n_users, self.n_items)
        mapped = self._mapped()
        if builder == "auto" and not mapped and _FAST_BACKOFF.get(self._backoff_key, 0) > 0:
            _FAST_BACKOFF[self._backoff_key] -= 1
            builder = "generic"
            self.fast_overflowed = True
        self._builder_arg = builder
        if builder == "small":
            self._build_small()
        if builder in ("auto", "fast") and not self._build_fast():
            if builder == "fast":
                raise abi.WhisprRecHipError("fast plan builder not applicable to this batch size")
        if self._tried is None:
            self._build_generic()
        self._queue_readback()
        if not defer:
            self.finish()
            if validate:
                self.validate()

    # ------------------------------------------------------------------ builders (enqueue only)
    def _mapped(self):
        bm = self._bucket_map
        return bm is not None and (bm.users is not None or bm.items is not None) and bm.batch_size == self.batch_size

    def _build_fast(self):
        """enqueue the hand-written builder (+ hot-run scan); False when it does not apply to this shape"""
        L = abi.lib()
        u, p, n = self._src
        dt, dev = u.dtype, u.device
        args = (self.n_triplets, self.batch_size, self.n_users, self.n_items)
        mapped = self._mapped()
        if mapped:
            mu, mi = self._bucket_map.users, self._bucket_map.items      # a side without a map keeps its equal-width buckets
            nbytes = abi.check_size(L.wr_bprmf_plan_fast_mapped_workspace_bytes(*args, mu["n_buckets"] if mu else 0,
                                                                                mi["n_buckets"] if mi else 0),
                                    "wr_bprmf_plan_fast_mapped_workspace_bytes")
        else:
            nbytes = abi.check_size(L.wr_bprmf_plan_fast_workspace_bytes(*args), "wr_bprmf_plan_fast_workspace_bytes")
        if nbytes <= 0:
            return False
        ws = workspace(dev, self._ws_tag + ("_fastmap" if mapped else "_fast")).get(nbytes)
        if self._want_hot:
            self._sides = self._hot_arrays(dev)      # before the plan kernels: no host-side allocation between build and scan
        outs = (_p(self.tu), _p(self.tp), _p(self.tn), _p(self.torig), _p(self.oc_item), _p(self.oc_src), _p(self.flags),
                _p(ws), ws.numel(), _stream())
        self._bitmap_ready = False
        if self._want_overlap and not mapped and L.wr_bprmf_plan_fast_marks_supported(*args):
            # the item-sort workgroups write the batch's "several occurrences" bitmap themselves (no global atomics)
            fn = L.wr_bprmf_plan_build_fast_marks_i64 if dt == torch.int64 else L.wr_bprmf_plan_build_fast_marks_i32
            abi.check(fn(_p(u), _p(p), _p(n), *args, *outs[:-1], _p(self.arena.overlap["bitmap"]), _stream()),
                      "wr_bprmf_plan_build_fast_marks")
            self._bitmap_ready = True
        elif mapped:
            fn = L.wr_bprmf_plan_build_fast_mapped_i64 if dt == torch.int64 else L.wr_bprmf_plan_build_fast_mapped_i32
            abi.check(fn(_p(u), _p(p), _p(n), *args, ctypes.addressof(mu["struct"]) if mu else None,
                         ctypes.addressof(mi["struct"]) if mi else None, *outs), "wr_bprmf_plan_build_fast_mapped")
        else:
            fn = L.wr_bprmf_plan_build_fast_i64 if dt == torch.int64 else L.wr_bprmf_plan_build_fast_i32
            abi.check(fn(_p(u), _p(p), _p(n), *args, *outs), "wr_bprmf_plan_build_fast")
        self._tried = "fast+map" if mapped else "fast"
        # the hot-run scan is bounds-safe for any key values; after an overflow its output is thrown away with the plan
        if self._want_hot:
            self._enqueue_hot_runs()
        if self._want_overlap:
            self._enqueue_overlap_marks()
        return True

    def _build_small(self):
        """one launch, one workgroup per batch (batch_size <= 4,096): nothing to read back but the index-range flag"""
        L = abi.lib()
        u, p, n = self._src
        if self.batch_size > int(L.wr_bprmf_plan_small_max_batch()):
            raise abi.WhisprRecHipError("small plan builder: batch size %d > %d" % (self.batch_size,
                                                                                    L.wr_bprmf_plan_small_max_batch()))
        fn = L.wr_bprmf_plan_build_small_i64 if u.dtype == torch.int64 else L.wr_bprmf_plan_build_small_i32
        abi.check(fn(_p(u), _p(p), _p(n), self.n_triplets, self.batch_size, self.n_users, self.n_items, _p(self.tu), _p(self.tp),
                     _p(self.tn), _p(self.torig), _p(self.oc_item), _p(self.oc_src), None if self._unchecked else _p(self.err),
                     _stream()), "wr_bprmf_plan_build_small")
        self.builder = self._tried = "small"
        self._bitmap_ready = False
        if self._want_hot:
            self._sides = self._hot_arrays(u.device)
            self._enqueue_hot_runs()
        if self._want_overlap:
            self._enqueue_overlap_marks()

    def _build_generic(self):
        L = abi.lib()
        u, p, n = self._src
        dev = u.device
        args = (self.n_triplets, self.batch_size, self.n_users, self.n_items)
        nbytes = abi.check_size(L.wr_bprmf_plan_workspace_bytes(*args), "wr_bprmf_plan_workspace_bytes")
        ws = workspace(dev, self._ws_tag).get(nbytes)  # distinct tags allow plan builds in flight on different streams
        fn = L.wr_bprmf_plan_build_i64 if u.dtype == torch.int64 else L.wr_bprmf_plan_build_i32
        abi.check(fn(_p(u), _p(p), _p(n), *args, _p(self.tu), _p(self.tp), _p(self.tn), _p(self.torig),
                     _p(self.oc_item), _p(self.oc_src), _p(self.err), _p(ws), ws.numel(), _stream()),
                  "wr_bprmf_plan_build")
        self.builder = "generic"
        self._tried = "generic"
        self._bitmap_ready = False
        if self._want_hot:
            if self._sides is None:
                self._sides = self._hot_arrays(dev)
            self._enqueue_hot_runs()
        if self._want_overlap:
            self._enqueue_overlap_marks()

    def _hot_arrays(self, dev):
        """list arrays of the hot-run scan: views of the arena, or fresh tensors"""
        i32 = dict(dtype=torch.int32, device=dev)
        nb = self.n_batches
        sides = []
        for kind in (0, 1):
            if self.arena is not None:
                buf, cp, cr = self.arena.hot_sides[kind]
                m = self.arena.max_batches
                arrs = [buf[:nb * cp], buf[m * cp:m * cp + nb * cp], buf[2 * m * cp:2 * m * cp + nb * cr],
                        buf[2 * m * cp + m * cr:2 * m * cp + m * cr + nb * cr],
                        buf[2 * m * cp + 2 * m * cr:2 * m * cp + 2 * m * cr + nb * cr]]
            else:
                cp, cr = hot_caps(self.batch_size, kind)
                arrs = [torch.empty(nb * cp, **i32), torch.empty(nb * cp, **i32), torch.empty(nb * cr, **i32),
                        torch.empty(nb * cr, **i32), torch.empty(nb * cr, **i32)]
            sides.append((arrs, cp, cr))
        return sides

    def _enqueue_hot_runs(self):
        """Cuts table rows with more than 32 occurrences in a batch (item rows: runs of oc_item; user rows: runs of tu) into
        pieces for the many-workgroup path (power-law ids); the per-batch counts travel with the plan's flags."""
        L = abi.lib()
        counts = self.meta[self.META_HEAD:self.META_HEAD + 4 * self.n_batches]
        for (kind, keys), (arrs, _, _) in zip(((0, self.oc_item), (1, self.tu)), self._sides):
            abi.check(L.wr_bprmf_plan_hot_runs(_p(keys), kind, self.n_triplets, self.batch_size, *[_p(a) for a in arrs],
                                               _p(counts), _stream()), "wr_bprmf_plan_hot_runs")

    def _enqueue_overlap_marks(self):
        """marks of the overlapped step stream: which user runs of batch k+1 read an item row that step k's item phase
        rewrites (index work only).  The first batch of a plan defers nothing: the stream joins at plan boundaries."""
        o, cb = self.arena.overlap, self._cap_batches
        counts = self.meta[self.META_HEAD + 4 * cb:self.META_HEAD + 5 * cb]
        L = abi.lib()
        fn = L.wr_bprmf_plan_overlap_deferred if getattr(self, "_bitmap_ready", False) else L.wr_bprmf_plan_overlap_marks
        abi.check(fn(_p(self.tu), _p(self.tp), _p(self.tn), self.n_triplets, self.batch_size, self.n_items, None,
                     _p(o["bitmap"]), _p(o["tdef"]), _p(o["def_q"]), o["cap"], _p(counts), _stream()),
                  "wr_bprmf_plan_overlap_marks")

    def _queue_readback(self):
        """ONE small read-back per plan: flags + hot-run counts (+ deferred-run counts).  With an arena it is an asynchronous
        copy into pinned memory and an event; finish() waits for the event."""
        if self._pinned is not None:
            self._pinned.copy_(self.meta, non_blocking=True)
            self.ready = torch.cuda.Event()
            self.ready.record(self._stream)

    # ------------------------------------------------------------------ host-side completion
    def _read_meta(self):
        if self._pinned is not None:
            self.ready.synchronize()
            return self._pinned
        return self.meta.cpu()

    def finish(self):
        """Makes the plan's host-side state final: waits for the read-back (no wait at all once the build has run, which is
        the normal case one chunk ahead of the steps), falls back to the radix-sort builder after a bucket overflow, and
        publishes the hot-run counts.  Idempotent.  A plan that has nothing to report (radix-sort builder, no hot-run scan)
        is finished without any device-to-host traffic; its index-range flag is read by validate() on demand."""
        if self._finished:
            return self
        mh = None
        while self._tried in ("fast", "fast+map") or self._want_hot:
            mh = self._read_meta()
            overflow = int(self.arena.meta_np[1]) if self._pinned is not None else int(mh[1])
            if self._tried in ("fast", "fast+map") and overflow != 0:
                if self._builder_arg == "fast":
                    raise abi.WhisprRecHipError("fast plan builder: bucket overflow (skewed ids)")
                self.fast_overflowed = True
                if self._tried == "fast":
                    _FAST_BACKOFF[self._backoff_key] = 32
                with torch.cuda.stream(self._stream):        # rebuild where the plan was built (rare: skewed ids without a map)
                    self.meta.zero_()
                    self._build_generic()
                    self._queue_readback()
                mh = None                                    # stale: the rebuilt plan reports again
                continue
            break
        self.meta_host = mh
        if self.builder is None:
            self.builder = self._tried
        if self._want_hot:
            if self._pinned is not None:
                any_hot = bool(self.arena.meta_np[self.META_HEAD:self.META_HEAD + 4 * self.n_batches].any())
            else:
                any_hot = int(mh[self.META_HEAD:self.META_HEAD + 4 * self.n_batches].sum().item()) > 0
            if any_hot:
                self.hot = {"sides": self._sides, "counts_host": mh[self.META_HEAD:self.META_HEAD + 4 * self.n_batches]}
        if self._want_overlap and self.hot is None:
            o, nb, cb = self.arena.overlap, self.n_batches, self._cap_batches
            # views of the arena's words, made once per (arena, plan length): this runs on the step path, between a plan's
            # read-back and its first launch
            views = self.arena.views.get((nb, cb))
            if views is None:
                lo = self.META_HEAD + 4 * cb
                views = self.arena.views[(nb, cb)] = (mh[lo:lo + nb], self.arena.meta_np[lo:lo + nb], self.meta[lo:lo + cb])
            dc, dcn, dcd = views
            lo_n, hi_n = (int(dcn.min()), int(dcn.max())) if nb >= 2 else (-1, -1)
            if nb >= 2 and lo_n >= 0:
                # "fits": every batch's list of deferred runs is within capacity (the two-stream form needs that; the
                # chained launch decides per step)
                self.overlap = {"tdef": o["tdef"], "def_q": o["def_q"], "def_count_host": dc, "cap": o["cap"],
                                "def_count_np": dcn, "fits": hi_n <= o["cap"], "def_count_dev": dcd}
        self._finished = True
        return self

    def hot_struct(self, batch=None):
        """ctypes wr_hot_runs for the whole plan (batch=None) or for one batch; None when the plan has no hot runs."""
        self.finish()
        if self.hot is None:
            return None
        k = 0 if batch is None else batch
        vals = []
        for arrs, cp, cr in self.hot["sides"]:
            vals += [arrs[0].data_ptr() + 4 * k * cp, arrs[1].data_ptr() + 4 * k * cp, arrs[2].data_ptr() + 4 * k * cr,
                     arrs[3].data_ptr() + 4 * k * cr, arrs[4].data_ptr() + 4 * k * cr]
        (_, cp0, cr0), (_, cp1, cr1) = self.hot["sides"]
        return abi.HotRuns(*vals, self.hot["counts_host"].data_ptr() + 16 * k, cp0, cr0, cp1, cr1)

    def validate(self):
        """nn.Embedding raises IndexError for out-of-range ids; so does the plan."""
        if self._unchecked:
            raise abi.WhisprRecHipError("this plan was built with validate=False and keeps no index-range flag")
        self.finish()
        if self.meta_host is None:
            self.meta_host = self._read_meta()
        bad = int(self.arena.meta_np[0]) if self._pinned is not None else int(self.meta_host[0].item())
        if bad != 0:
            raise IndexError("index out of range in batch (user_id >= n_users or item id >= n_items)")

    def batch_len(self, k):
        return min(self.batch_size, self.n_triplets - k * self.batch_size)

    def record_stream(self, stream):
        """A plan built on a side stream and consumed on `stream`: tell the caching allocator, so that dropping the plan
        while its steps are still queued does not hand the arrays to the next build.  (Arena plans: PlanArena.release_after.)"""
        if self.arena is not None:
            return
        ts = [self.tu, self.tp, self.tn, self.oc_item, self.oc_src, self.meta]
        if self.torig is not None:
            ts.append(self.torig)
        if self._sides is not None:
            for arrs, _, _ in self._sides:
                ts += arrs
        for t in ts:
            t.record_stream(stream)


class GroupArena:
    """Pre-sized home of ONE group plan (GroupPlan): the plan words and the pinned mirror of its meta words.  Like
    PlanArena: nothing is allocated while steps run, the read-back is an asynchronous copy consumed at first use."""

    def __init__(self, device, max_triplets, batch_size, n_users, n_items):
        words = int(abi.lib().wr_group_plan_words(int(max_triplets), int(batch_size), int(n_users), int(n_items)))
        if words <= 0:
            raise abi.WhisprRecHipError("group plan: shape not supported (batch size %d)" % batch_size)
        self.device, self.max_triplets, self.batch_size = device, int(max_triplets), int(batch_size)
        self.n_users, self.n_items = int(n_users), int(n_items)
        self.buf = torch.empty(words, dtype=torch.int32, device=device)
        self.meta_host = torch.zeros(GroupPlan.META, dtype=torch.int32, pin_memory=True)
        self.meta_np = self.meta_host.numpy()
        self.free = None

    def release_after(self, stream):
        self.free = torch.cuda.Event()
        self.free.record(stream)


class GroupPlan:
    """Batches for the step stream WITHOUT a per-batch sort (include/whisprrec_hip.h, wr_group_plan_build): the triplets stay
    where they are (``u, p, n`` int32, batch order — kept by the plan, the step kernels read them); per batch the plan holds
    four flag bits per triplet and the shared occurrences only, as sorted lists.  One launch per build, ~0.1 B of plan per
    triplet.  ``finish()`` publishes ``bad_index`` / ``overflow`` (the plan is unusable: fall back to BatchPlan) /
    ``long_run`` (usable, but a row has more than 64 occurrences in a batch)."""

    META = 16

    def __init__(self, u, p, n, batch_size, n_users, n_items, arena=None, defer=False):
        u, p, n = (_req(t, torch.int32, nm, 1) for t, nm in ((u, "u"), (p, "p"), (n, "n")))
        N = u.numel()
        if not (p.numel() == N and n.numel() == N) or N == 0:
            raise ValueError("u/p/n must have the same non-zero length")
        L = abi.lib()
        self.u, self.p, self.n = u, p, n
        self.n_triplets, self.batch_size = N, int(batch_size)
        self.n_users, self.n_items = int(n_users), int(n_items)
        self.n_batches = (N + self.batch_size - 1) // self.batch_size
        self.words = int(L.wr_group_plan_words(N, self.batch_size, self.n_users, self.n_items))
        if self.words <= 0:
            raise abi.WhisprRecHipError("group plan: shape not supported (batch size %d)" % self.batch_size)
        self.arena = arena
        self._stream = torch.cuda.current_stream(u.device)
        if arena is not None:
            if arena.buf.numel() < self.words or arena.batch_size != self.batch_size or \
                    (arena.n_users, arena.n_items) != (self.n_users, self.n_items):
                raise ValueError("plan does not fit its arena")
            if arena.free is not None:
                self._stream.wait_event(arena.free)
                arena.free = None
            self.buf = arena.buf
            self._pinned = arena.meta_host
        else:
            self.buf = torch.empty(self.words, dtype=torch.int32, device=u.device)
            self._pinned = None
        abi.check(L.wr_group_plan_build(_p(u), _p(p), _p(n), N, self.batch_size, self.n_users, self.n_items, _p(self.buf),
                                        self.buf.numel(), _stream()), "wr_group_plan_build")
        self.ready = None
        if self._pinned is not None:
            self._pinned.copy_(self.buf[:self.META], non_blocking=True)
            self.ready = torch.cuda.Event()
            self.ready.record(self._stream)
        self._finished = False
        self.bad_index = self.overflow = self.long_run = False
        if not defer:
            self.finish()

    def finish(self):
        if self._finished:
            return self
        if self._pinned is not None:
            self.ready.synchronize()
            m = self.arena.meta_np
        else:
            m = self.buf[:self.META].cpu().numpy()
        self.bad_index, self.overflow, self.long_run = bool(m[0]), bool(m[1]), bool(m[2])
        self._finished = True
        return self

    def finish_from(self, meta):
        """the plan's first three words, read back by the caller together with words of its own"""
        self.bad_index, self.overflow, self.long_run = bool(meta[0]), bool(meta[1]), bool(meta[2])
        self._finished = True
        return self

    def validate(self):
        """nn.Embedding raises IndexError for out-of-range ids; so does the plan."""
        self.finish()
        if self.bad_index:
            raise IndexError("index out of range in batch (user_id >= n_users or item id >= n_items)")

    def batch_len(self, k):
        return min(self.batch_size, self.n_triplets - k * self.batch_size)

    def layout(self):
        out = (ctypes.c_int64 * 16)()
        abi.check(abi.lib().wr_group_plan_layout(self.n_triplets, self.batch_size, self.n_users, self.n_items,
                                                 ctypes.addressof(out)), "wr_group_plan_layout")
        keys = ("nb", "fw", "R_u", "R_i", "mask_u", "mask_i", "flags", "ucnt", "icnt", "ul_row", "ul_src", "il_row", "il_src",
                "total", "cap_u", "cap_i")
        return dict(zip(keys, [int(v) for v in out]))

    def decode(self):
        """the plan as NumPy arrays (tests, statistics): flags [nb, fw, 4] uint32 and, per (batch, range), the user and item
        lists as (rows, sources)"""
        import numpy as np
        self.finish()
        Ly = self.layout()
        w = self.buf[:Ly["total"]].cpu().numpy()
        nb, fw = Ly["nb"], Ly["fw"]
        flags = w[Ly["flags"]:Ly["flags"] + nb * fw * 4].view(np.uint32).reshape(nb, fw, 4).copy()
        out = {"flags": flags, "users": {}, "items": {}, "R_u": Ly["R_u"], "R_i": Ly["R_i"], "meta": w[:self.META].copy()}
        for side, R, cap, co, ro, so in (("users", Ly["R_u"], Ly["cap_u"], "ucnt", "ul_row", "ul_src"),
                                         ("items", Ly["R_i"], Ly["cap_i"], "icnt", "il_row", "il_src")):
            for b in range(nb):
                for r in range(R):
                    c = int(w[Ly[co] + b * R + r])
                    at = (b * R + r) * cap
                    out[side][(b, r)] = (w[Ly[ro] + at:Ly[ro] + at + c].astype(np.int64),
                                         w[Ly[so] + at:Ly[so] + at + c].astype(np.int64))
        return out


_CHAIN_SYNC = {}      # (device, stream) -> [int32 tensors]: hand-off counters of the chained step launches (BprmfTables._chain_sync)
_OVERLAP_WS_BYTES = {}       # (batch size, D) -> bytes of the two-slot step workspace


class BprmfTables:
    """The two embedding tables plus the scratch the step kernels need.  Tables are plain fp32 tensors
    (row-major [n_rows, D]) that stay valid PyTorch tensors between steps."""

    def __init__(self, user_tab, item_tab):
        self.U = _req(user_tab, torch.float32, "user_tab", 2)
        self.I = _req(item_tab, torch.float32, "item_tab", 2)
        if self.U.shape[1] != self.I.shape[1]:
            raise ValueError("user and item tables must have the same embedding size")
        self.D = self.U.shape[1]
        self.dev = self.U.device
        self.stamp_u = None
        self.stamp_i = None
        self.step_id = 0

    def _stamps(self):
        if self.stamp_u is None:
            self.stamp_u = torch.full((self.U.shape[0],), -1, dtype=torch.int32, device=self.dev)
            self.stamp_i = torch.full((self.I.shape[0],), -1, dtype=torch.int32, device=self.dev)
        return self.stamp_u, self.stamp_i

    def _ws(self, B):
        nbytes = abi.check_size(abi.lib().wr_bprmf_step_workspace_bytes(B, self.D), "wr_bprmf_step_workspace_bytes")
        return workspace(self.dev, "step").get(nbytes)

    def _loss_buf(self, out, count=None):
        """the caller's loss tensor, or a new one: a scalar, or one float per step"""
        return out if out is not None else torch.empty(() if count is None else count, dtype=torch.float32, device=self.dev)

    def _table_head(self):
        """(U, n_users, I, n_items, D): how every step entry's argument list starts"""
        return (_p(self.U), self.U.shape[0], _p(self.I), self.I.shape[0], self.D)

    @staticmethod
    def _plan_head(plan):
        """(tu, tp, tn, oc_item, oc_src, n_triplets, batch_size): the sorted plan in the run entries' argument lists"""
        return (_p(plan.tu), _p(plan.tp), _p(plan.tn), _p(plan.oc_item), _p(plan.oc_src), plan.n_triplets, plan.batch_size)

    def _plan_ptrs(self, plan, k):
        """(tu, tp, tn, oc_item, oc_src, B) of batch k: the plan in the single-step entries' argument lists"""
        off = k * plan.batch_size
        return (plan.tu.data_ptr() + 4 * off, plan.tp.data_ptr() + 4 * off, plan.tn.data_ptr() + 4 * off,
                plan.oc_item.data_ptr() + 8 * off, plan.oc_src.data_ptr() + 8 * off, plan.batch_len(k))

    def step_sgd(self, plan, k, lr, l2=0.0, loss_out=None, decay_untouched=True):
        """One BaseRunner.fit iteration (zero_grad/predict/backward/SGD.step, BaseRunner.py:196-199) on batch k.
        decay_untouched=False leaves the weight decay of the rows outside the batch to LazyOptimizerState."""
        L = abi.lib()
        ws = self._ws(plan.batch_size)
        loss_out = self._loss_buf(loss_out)
        su = si = None
        self.step_id += 1
        if l2 != 0.0:
            su, si = self._stamps()
        hot = plan.hot_struct(k)
        abi.check(L.wr_bprmf_step_sgd(*self._table_head(), *self._plan_ptrs(plan, k), lr, l2, _p(su), _p(si), self.step_id,
                                      _p(loss_out), _addr(hot), _p(ws), ws.numel(), _stream()), "wr_bprmf_step_sgd")
        if l2 != 0.0 and decay_untouched:  # dense weight decay on the rows the batch did not touch (torch.optim.SGD semantics)
            abi.check(L.wr_sgd_decay_untouched(_p(self.U), self.U.shape[0], self.D, _p(su), self.step_id, lr, l2,
                                               _stream()), "wr_sgd_decay_untouched")
            abi.check(L.wr_sgd_decay_untouched(_p(self.I), self.I.shape[0], self.D, _p(si), self.step_id, lr, l2,
                                               _stream()), "wr_sgd_decay_untouched")
        return loss_out

    def run_sgd(self, plan, first, count, lr, losses=None, phase_events=None):
        """`count` consecutive steps starting at batch `first` (native inner loop of BaseRunner.fit, l2 = 0).

        phase_events: optional list of 4*count ``torch.cuda.Event(enable_timing=True)`` or None entries: per step the
        start / stop events of its two phases (include/whisprrec_hip.h; bench.py's per-kernel timing)."""
        L = abi.lib()
        ws = self._ws(plan.batch_size)
        losses = self._loss_buf(losses, count)
        hot = plan.hot_struct()
        ev = _event_handles(phase_events, 4, count, True)
        abi.check(L.wr_bprmf_run_sgd(*self._table_head(), *self._plan_head(plan), first, count, lr, _p(losses), _addr(ev),
                                     _addr(hot), _p(ws), ws.numel(), _stream()), "wr_bprmf_run_sgd")
        self.step_id += count
        return losses

    def overlap_workspace(self, batch_size):
        nbytes = _OVERLAP_WS_BYTES.get((batch_size, self.D))
        if nbytes is None:
            nbytes = _OVERLAP_WS_BYTES[(batch_size, self.D)] = 2 * abi.check_size(
                abi.lib().wr_bprmf_step_workspace_bytes(batch_size, self.D), "wr_bprmf_step_workspace_bytes")
        return workspace(self.dev, "step_overlap").get(nbytes)

    def chain_supported(self):
        """rows are whole 128-byte lines (D % 32 == 0, tables 128-byte aligned): the chained step launch applies"""
        return bool(abi.lib().wr_bprmf_chain_supported(_p(self.U), _p(self.I), self.D))

    CHAIN_SYNC_STEPS = 256      # the hand-off counters are sized for calls of this many steps up front (1 MB): growing
                                # them means an allocation in the middle of a step stream

    def _chain_sync(self, count):
        """hand-off counters + sticky timeout word of the chained launches: ONE buffer per (device, stream) shared by every
        tables object (the stratified schedule makes one per segment) — calls on a stream are ordered, each zeroes the
        counters it uses"""
        key = (str(self.dev), torch.cuda.current_stream(self.dev).cuda_stream)
        bufs = _CHAIN_SYNC.setdefault(key, [])
        if bufs and count <= self.CHAIN_SYNC_STEPS:
            return bufs[-1]                              # sized for CHAIN_SYNC_STEPS steps or more
        if not bufs or bufs[-1].numel() < int(abi.lib().wr_bprmf_chain_sync_words(count)):
            words = int(abi.lib().wr_bprmf_chain_sync_words(max(count, self.CHAIN_SYNC_STEPS)))
            bufs.append(torch.zeros(words, dtype=torch.int32, device=self.dev))      # older ones stay for check_chain
        return bufs[-1]

    def sticky_words(self):
        """the sticky "a bounded wait expired" words of the step launches issued on the current stream of this device (one
        int32 view per hand-off buffer) — PipelinedSgd copies them to pinned memory behind every chunk"""
        sid = torch.cuda.current_stream(self.dev).cuda_stream
        return [buf[-4:-3] for key, bufs in _CHAIN_SYNC.items() if key[0] == str(self.dev) and key[1] == sid for buf in bufs]

    def check_chain(self):
        """raises if a bounded wait inside a chained step launch ever expired on this device (synchronises; call it where
        the caller waits for the device anyway: end of an epoch, end of a benchmark)"""
        for key, bufs in _CHAIN_SYNC.items():
            if key[0] != str(self.dev):
                continue
            for buf in bufs:
                if int(buf[-4].item()) != 0:
                    raise abi.WhisprRecHipError("chained step launch: a wait for the item tiles expired — the tables are "
                                                "not valid")

    def run_sgd_chain(self, plan, first, count, lr, losses=None, phase_events=None, ws=None, def_limit=None):
        """`count` consecutive steps like run_sgd, one launch per step (wr_bprmf_run_sgd_chain): the item phase of step k-1
        rides in the launch of step k's user phase.  plan.overlap must be set (BatchPlan built with overlap=True that
        qualified: no hot rows, deferred-run lists within capacity).  Same tables, bit for bit, as run_sgd."""
        L = abi.lib()
        o = plan.overlap
        if ws is None:
            ws = self.overlap_workspace(plan.batch_size)
        losses = self._loss_buf(losses, count)
        ev = _event_handles(phase_events, 4, count, True)
        sync = self._chain_sync(count)
        abi.check(L.wr_bprmf_run_sgd_chain(*self._table_head(), *self._plan_head(plan), first, count, lr, _p(losses),
                                           _p(o["tdef"]), _p(o["def_q"]), o["def_count_host"].data_ptr(), o["cap"],
                                           o["cap"] if def_limit is None else int(def_limit), _addr(ev), _p(ws), ws.numel(),
                                           _p(sync), sync.numel(), _stream()), "wr_bprmf_run_sgd_chain")
        self.step_id += count
        return losses

    def group_supported(self):
        """rows are whole 128-byte lines: the step stream without a per-batch sort applies (wr_bprmf_run_sgd_group)"""
        return bool(abi.lib().wr_bprmf_group_supported(_p(self.U), _p(self.I), self.D))

    def _group_sync(self, count):
        """hand-off counters + sticky timeout word of wr_bprmf_run_sgd_group: kept with the chained launches' (check_chain
        reads both)"""
        key = (str(self.dev), torch.cuda.current_stream(self.dev).cuda_stream, "group")
        bufs = _CHAIN_SYNC.setdefault(key, [])
        need = int(abi.lib().wr_bprmf_group_sync_words(count))
        if not bufs or bufs[-1].numel() < need:
            words = int(abi.lib().wr_bprmf_group_sync_words(max(count, self.CHAIN_SYNC_STEPS)))
            bufs.append(torch.zeros(words, dtype=torch.int32, device=self.dev))
        return bufs[-1]

    def run_sgd_group(self, gplan, first, count, lr, losses=None, events=None):
        """`count` consecutive steps of a GroupPlan from batch `first` (wr_bprmf_run_sgd_group): one launch per step, no
        sorted plan.  events: optional 2 * count ``torch.cuda.Event(enable_timing=True)`` — start / stop of each step's launch."""
        L = abi.lib()
        nbytes = abi.check_size(L.wr_bprmf_group_workspace_bytes(gplan.batch_size, self.D), "wr_bprmf_group_workspace_bytes")
        ws = workspace(self.dev, "group_step").get(nbytes)
        losses = self._loss_buf(losses, count)
        ev = _event_handles(events, 2, count, False)
        sync = self._group_sync(count)
        abi.check(L.wr_bprmf_run_sgd_group(*self._table_head(), _p(gplan.u), _p(gplan.p), _p(gplan.n), gplan.n_triplets,
                                           gplan.batch_size, _p(gplan.buf), gplan.buf.numel(), first, count, lr, _p(losses),
                                           _addr(ev), _p(ws), ws.numel(), _p(sync), sync.numel(), _stream()),
                  "wr_bprmf_run_sgd_group")
        self.step_id += count
        return losses

    def grads(self, plan, k, grad_u, grad_i, loss_out=None, stamps=True):
        """embedding_dense_backward of BaseRunner.py:198 for batch k: writes the gradient rows of the rows in the
        batch into grad_u / grad_i and stamps them with the returned step id (other rows are not written).
        stamps=False: no stamp arrays at all — for a caller that zero-filled grad_u / grad_i and reads them densely."""
        L = abi.lib()
        ws = self._ws(plan.batch_size)
        su, si = self._stamps() if stamps else (None, None)
        loss_out = self._loss_buf(loss_out)
        self.step_id += 1
        hot = plan.hot_struct(k)
        abi.check(L.wr_bprmf_grads(*self._table_head(), *self._plan_ptrs(plan, k), _p(grad_u), _p(grad_i), _p(su), _p(si),
                                   self.step_id, _p(loss_out), _addr(hot), _p(ws), ws.numel(), _stream()), "wr_bprmf_grads")
        return loss_out, self.step_id


# ----------------------------------------------------------------------------------------------- epoch prep
PAIR_SET_MIN_PAIRS = 1 << 20      # from this many (user, item) pairs on the samplers test membership in a hash set


def pair_set(clicked_ptr, clicked_idx, n_users):
    """Hash set of the (user, item) pairs of the clicked lists (wr_pairset_build): int64 tensor [capacity] for the `pairs`
    argument of sample_negatives / EpochPrep.  One membership test = one random 64-byte sector instead of a binary search
    in the user's list (~7 sectors): same answers, same negatives.  Built once per training frame."""
    _req(clicked_ptr, torch.int64, "clicked_ptr", 1)
    _req(clicked_idx, torch.int32, "clicked_idx", 1)
    L = abi.lib()
    cap = abi.check_size(L.wr_pairset_capacity(int(clicked_idx.numel())), "wr_pairset_capacity")
    table = torch.empty(cap, dtype=torch.int64, device=clicked_ptr.device)
    err = torch.zeros(1, dtype=torch.int32, device=clicked_ptr.device)
    abi.check(L.wr_pairset_build(_p(clicked_ptr), _p(clicked_idx), int(n_users), _p(table), cap, _p(err), _stream()),
              "wr_pairset_build")
    if int(err.item()) != 0:
        raise abi.WhisprRecHipError("pair set: table too small")
    return table


def sample_negatives(users, n_users, n_items, clicked_ptr, clicked_idx, seed, epoch, pairs=None):
    """Device negative sampler (reference src/models/BaseModel.py:167-177 semantics, counter-based generator).
    pairs: pair_set(clicked_ptr, clicked_idx, n_users) — membership through the hash set instead of the lists."""
    if users.dtype not in (torch.int64, torch.int32):
        raise TypeError("users must be int64 or int32")
    users = _req(users.contiguous(), users.dtype, "users", 1)
    if pairs is None:
        _req(clicked_ptr, torch.int64, "clicked_ptr", 1)
        _req(clicked_idx, torch.int32, "clicked_idx", 1)
    neg = torch.empty_like(users)
    err = torch.zeros(1, dtype=torch.int32, device=users.device)
    L = abi.lib()
    if pairs is not None:
        fn = L.wr_sample_negatives_set_i64 if users.dtype == torch.int64 else L.wr_sample_negatives_set_i32
        abi.check(fn(_p(users), users.numel(), n_users, n_items, _p(_req(pairs, torch.int64, "pairs", 1)), pairs.numel(), seed,
                     epoch, _p(neg), _p(err), _stream()), "wr_sample_negatives_set")
        return neg, err
    fn = L.wr_sample_negatives_i64 if users.dtype == torch.int64 else L.wr_sample_negatives_i32
    abi.check(fn(_p(users), users.numel(), n_users, n_items, _p(clicked_ptr), _p(clicked_idx), seed, epoch, _p(neg), _p(err),
                 _stream()), "wr_sample_negatives")
    return neg, err


def epoch_shuffle(cols, seed, epoch, want_order=False):
    """Device epoch shuffle (wr_epoch_shuffle): up to three 1-D index columns of one dtype (int64 or int32) and one length,
    permuted by the same keyed bijection of the rows.  Returns the permuted columns (and the int64 order if asked)."""
    cols = list(cols)
    if not 1 <= len(cols) <= 3:
        raise ValueError("one to three columns")
    dt = cols[0].dtype
    if dt not in (torch.int64, torch.int32):
        raise TypeError("columns must be int64 or int32")
    n = cols[0].numel()
    cols = [_req(c.contiguous(), dt, "column", 1) for c in cols]
    if any(c.numel() != n for c in cols):
        raise ValueError("columns must have the same length")
    outs = [torch.empty_like(c) for c in cols]
    order = torch.empty(n, dtype=torch.int64, device=cols[0].device) if want_order else None
    pad = [None] * (3 - len(cols))
    fn = abi.lib().wr_epoch_shuffle_i64 if dt == torch.int64 else abi.lib().wr_epoch_shuffle_i32
    abi.check(fn(*[_p(c) for c in cols + pad], n, int(seed), int(epoch), *[_p(o) for o in outs + pad], _p(order), _stream()),
              "wr_epoch_shuffle")
    return (outs, order) if want_order else outs


class EpochPrep:
    """The epoch's (user, positive, negative) columns in batch order, produced RANGE BY RANGE on the device
    (wr_epoch_prepare_range: keyed shuffle + negative sampling fused; same columns as sample_negatives + epoch_shuffle).
    ``cols`` are the epoch-sized output arrays; ``fill(lo, hi)`` enqueues rows [lo, hi) on the current stream.  PipelinedSgd
    calls it for each plan chunk right before that chunk's plan build, on the plan stream: the preparation of chunk c+1 runs
    beside the steps of chunk c."""

    def __init__(self, users, items, n_users, n_items, clicked_ptr, clicked_idx, seed, epoch, want_order=False, pairs=None,
                 packed=None):
        """pairs: pair_set(...) — membership through the hash set; packed: pack_rows(users, items) — with a pair set, the
        source rows are read as one 8-byte word each (one random sector per output row instead of two; same columns)"""
        if users.dtype not in (torch.int64, torch.int32) or items.dtype != users.dtype:
            raise TypeError("users / items must both be int64 or int32")
        self.users = _req(users.contiguous(), users.dtype, "users", 1)
        self.items = _req(items.contiguous(), users.dtype, "items", 1)
        if self.items.numel() != self.users.numel():
            raise ValueError("users / items must have the same length")
        if pairs is None:
            _req(clicked_ptr, torch.int64, "clicked_ptr", 1)
            _req(clicked_idx, torch.int32, "clicked_idx", 1)
        self.ptr, self.idx = clicked_ptr, clicked_idx
        self.pairs = None if pairs is None else _req(pairs, torch.int64, "pairs", 1)     # pair_set(...): hash-set membership
        self.packed = None
        if packed is not None and pairs is not None:
            self.packed = _req(packed, torch.int64, "packed", 1)
            if self.packed.numel() != self.users.numel():
                raise ValueError("packed rows: one word per interaction")
        self.n, self.n_users, self.n_items = users.numel(), int(n_users), int(n_items)
        self.seed, self.epoch = int(seed), int(epoch)
        self.cols = [torch.empty_like(self.users) for _ in range(3)]
        self.order = torch.empty(self.n, dtype=torch.int64, device=users.device) if want_order else None
        self.err = torch.zeros(1, dtype=torch.int32, device=users.device)
        self.filled = 0

    def fill(self, lo, hi):
        lo, hi = int(lo), min(int(hi), self.n)
        if hi <= lo:
            return
        es = self.users.element_size()
        L = abi.lib()
        tail = (self.seed, self.epoch, lo, hi - lo, self.cols[0].data_ptr() + es * lo, self.cols[1].data_ptr() + es * lo,
                self.cols[2].data_ptr() + es * lo, None if self.order is None else self.order.data_ptr() + 8 * lo,
                _p(self.err), _stream())
        if self.packed is not None:
            fn = L.wr_epoch_prepare_range_packed_i64 if self.users.dtype == torch.int64 else L.wr_epoch_prepare_range_packed_i32
            abi.check(fn(_p(self.packed), self.n, self.n_users, self.n_items, _p(self.pairs), self.pairs.numel(), *tail),
                      "wr_epoch_prepare_range_packed")
        elif self.pairs is not None:
            fn = L.wr_epoch_prepare_range_set_i64 if self.users.dtype == torch.int64 else L.wr_epoch_prepare_range_set_i32
            abi.check(fn(_p(self.users), _p(self.items), self.n, self.n_users, self.n_items, _p(self.pairs), self.pairs.numel(),
                         *tail), "wr_epoch_prepare_range_set")
        else:
            fn = L.wr_epoch_prepare_range_i64 if self.users.dtype == torch.int64 else L.wr_epoch_prepare_range_i32
            abi.check(fn(_p(self.users), _p(self.items), self.n, self.n_users, self.n_items, _p(self.ptr), _p(self.idx), *tail),
                      "wr_epoch_prepare_range")
        self.filled = max(self.filled, hi)

    def check(self):
        """after the epoch (one read-back): nn.Embedding would have raised IndexError for an out-of-range user id"""
        if int(self.err.item()) == 1:
            raise IndexError("user id out of range in the training frame")


def pack_rows(users, items):
    """the training frame's (user, item) rows as one int64 word each, (user << 32) | item (EpochPrep(packed=...)); ids < 2^31"""
    return ((users.to(torch.int64) << 32) | items.to(torch.int64)).contiguous()


def clicked_csr_from_pairs(users, items, n_users, n_items):
    """device (user, item) interaction pairs -> device CSR of each user's distinct items, ascending (the layout
    wr_sample_negatives and wr_rank_eval take).  One-off setup: torch sort/unique glue."""
    key = torch.unique(users.to(torch.int64) * int(n_items) + items.to(torch.int64))      # sorted, distinct
    uu = torch.div(key, int(n_items), rounding_mode="floor")
    ptr = torch.zeros(n_users + 1, dtype=torch.int64, device=users.device)
    ptr[1:] = torch.cumsum(torch.bincount(uu, minlength=n_users), 0)
    return ptr, (key - uu * int(n_items)).to(torch.int32)


def clicked_csr(train_clicked_set, n_users, device):
    """train_clicked_set (dict user -> set of items, reference BaseReader.py:35-46) -> device CSR with ascending items."""
    import numpy as np
    ptr = np.zeros(n_users + 1, np.int64)
    chunks = []
    for uu in range(n_users):
        items = train_clicked_set.get(uu, ())
        ptr[uu + 1] = ptr[uu] + len(items)
        if len(items):
            chunks.append(np.sort(np.fromiter(items, dtype=np.int32, count=len(items))))
    idx = np.concatenate(chunks) if chunks else np.zeros(1, np.int32)
    return torch.from_numpy(ptr).to(device), torch.from_numpy(idx).to(device)


# ----------------------------------------------------------------------------------------------- evaluation
LDS_PER_WORKGROUP = 160 * 1024      # gfx950: 163,840 B per workgroup


def rank_eval_supports(D):
    """embedding sizes wr_rank_eval takes: the register-operand kernel for D in {8, 16, 32, 64}, otherwise the LDS-operand
    kernel, which stages (128 + 32) rows of D + 1 floats and 128 counters — D <= 252 on gfx950's 160 KiB of LDS"""
    D = int(D)
    if D % 4 != 0 or D < 4:
        return False
    return D in (8, 16, 32, 64) or ((128 + 32) * (D + 1) + 128) * 4 <= LDS_PER_WORKGROUP


def rank_eval(user_mat, item_tab, eval_user, eval_target, mask_ptr=None, mask_idx=None):
    """Rank of the ground-truth item among all (unmasked) items for every evaluation row (reference
    BaseRunner.interface + evaluate_method); returns (rank int32 [n], target_score fp32 [n]).  rank = 1 + the unmasked items
    scoring strictly above the target; a row whose target score is NaN ranks n_items + 1 (here, in rank_eval_rows and in
    rank_eval_multi alike)."""
    _req(user_mat, torch.float32, "user_mat", 2)
    _req(item_tab, torch.float32, "item_tab", 2)
    eu, et = _idx64(eval_user.reshape(-1), "eval_user"), _idx64(eval_target.reshape(-1), "eval_target")
    if mask_ptr is not None:
        _req(mask_ptr, torch.int64, "mask_ptr", 1)
        _req(mask_idx, torch.int32, "mask_idx", 1)
    n = eu.numel()
    rank = torch.empty(n, dtype=torch.int32, device=user_mat.device)
    tsc = torch.empty(n, dtype=torch.float32, device=user_mat.device)
    abi.check(abi.lib().wr_rank_eval(_p(user_mat), user_mat.shape[0], _p(item_tab), item_tab.shape[0], user_mat.shape[1],
                                     _p(eu), _p(et), n, _p(mask_ptr), _p(mask_idx), _p(rank), _p(tsc), _stream()),
              "wr_rank_eval")
    return rank, tsc


TOPK_MAX_K = 256
TOPK_WORKSPACE_CAP = 2 << 30        # bytes of workspace per call at most: the users go in blocks below it


def topk_supports(D, k):
    """(D, k) that wr_topk_recommend takes: 1 <= k <= 256 and the embedding sizes of rank_eval_supports"""
    return bool(abi.lib().wr_topk_supported(int(D), int(k)))


def _topk_blocks(n, n_items, D, k, dev, nbytes=None):
    """(lo, hi, workspace) for n rows in blocks whose workspace stays under TOPK_WORKSPACE_CAP (the bound never decreases in
    the row count: halve until it fits).  nbytes(rows): the bound of the entry that is called (wr_topk_workspace_bytes)"""
    L = abi.lib()

    if nbytes is None:
        def nbytes(rows):
            return abi.check_size(L.wr_topk_workspace_bytes(rows, n_items, D, k), "wr_topk_workspace_bytes")

    block = max(n, 1)
    while block > 128 and nbytes(block) > TOPK_WORKSPACE_CAP:
        block = (block + 1) // 2
    ws = workspace(dev, "topk")
    for lo in range(0, n, block):
        hi = min(n, lo + block)
        yield lo, hi, ws.get(nbytes(hi - lo))


def topk_recommend(user_mat, item_tab, users, k, mask_ptr=None, mask_idx=None):
    """The k unmasked items with the largest <user_mat[u], item_tab[j]> for every u in `users`, by score descending, then
    item id ascending (wr_topk_recommend).  Scores are bitwise those rank_eval computes.  Rows with fewer than k unmasked
    items end with item -1 / score -inf.  Returns (items int64 [n, k], scores float32 [n, k]) on the device."""
    _req(user_mat, torch.float32, "user_mat", 2)
    _req(item_tab, torch.float32, "item_tab", 2)
    qu = _idx64(users.reshape(-1), "users")
    if (mask_ptr is None) != (mask_idx is None):
        raise ValueError("mask_ptr and mask_idx go together")
    if mask_ptr is not None:
        _req(mask_ptr, torch.int64, "mask_ptr", 1)
        _req(mask_idx, torch.int32, "mask_idx", 1)
    k, D = int(k), int(user_mat.shape[1])
    if item_tab.shape[1] != D:
        raise ValueError("user_mat and item_tab have different widths (%d, %d)" % (D, item_tab.shape[1]))
    if not topk_supports(D, k):
        raise abi.WhisprRecHipError("topk_recommend does not support D=%d, k=%d (1 <= k <= %d; D as for rank_eval)"
                                    % (D, k, TOPK_MAX_K))
    L, dev = abi.lib(), user_mat.device
    n, n_items = qu.numel(), item_tab.shape[0]
    items = torch.empty((n, k), dtype=torch.int32, device=dev)
    scores = torch.empty((n, k), dtype=torch.float32, device=dev)
    for lo, hi, buf in _topk_blocks(n, n_items, D, k, dev):
        abi.check(L.wr_topk_recommend(_p(user_mat), user_mat.shape[0], _p(item_tab), n_items, D, _p(qu[lo:hi]), hi - lo,
                                      _p(mask_ptr), _p(mask_idx), k, _p(items[lo:hi]), _p(scores[lo:hi]), _p(buf),
                                      buf.numel(), _stream()),
                  "wr_topk_recommend")
    return items.to(torch.int64), scores


def _rows_args(fn, query_mat, item_tab, n, mask_row, mask_ptr, mask_idx, query_row):
    """the argument checks rank_eval_rows and topk_recommend_rows share -> (query_row, mask_row) as int64 or None"""
    if (mask_ptr is None) != (mask_idx is None):
        raise ValueError("mask_ptr and mask_idx go together")
    if (mask_ptr is None) != (mask_row is None):
        raise ValueError("%s: mask_row goes with mask_ptr and mask_idx (the row of the mask that each row uses)" % fn)
    _req(query_mat, torch.float32, "query_mat", 2)
    _req(item_tab, torch.float32, "item_tab", 2)
    if item_tab.shape[1] != query_mat.shape[1]:
        raise ValueError("query_mat and item_tab have different widths (%d, %d)" % (query_mat.shape[1], item_tab.shape[1]))
    if mask_ptr is not None:
        _req(mask_ptr, torch.int64, "mask_ptr", 1)
        _req(mask_idx, torch.int32, "mask_idx", 1)
        mask_row = _idx64(mask_row.reshape(-1), "mask_row")
    if query_row is not None:
        query_row = _idx64(query_row.reshape(-1), "query_row")
        n = query_row.numel() if n is None else n
        if query_row.numel() != n:
            raise ValueError("%s: query_row has %d entries for %d rows" % (fn, query_row.numel(), n))
    else:
        n = query_mat.shape[0] if n is None else n
        if n > query_mat.shape[0]:
            raise ValueError("%s: %d rows but query_mat has %d and no query_row is given" % (fn, n, query_mat.shape[0]))
    if mask_row is not None and mask_row.numel() != n:
        raise ValueError("%s: mask_row has %d entries for %d rows" % (fn, mask_row.numel(), n))
    return n, query_row, mask_row


def rank_eval_rows(query_mat, item_tab, eval_target, mask_row=None, mask_ptr=None, mask_idx=None, query_row=None):
    """rank_eval with one query vector per evaluation row (wr_rank_eval_rows; sequential models): row e scores with
    query_mat[query_row[e]] (query_row None: query_mat[e]) and is masked by the list of row mask_row[e] of the CSR
    mask_ptr / mask_idx — its user; several rows may share one.  Returns (rank int32 [n], target_score fp32 [n])."""
    n, qr, mr = _rows_args("rank_eval_rows", query_mat, item_tab, eval_target.numel(), mask_row, mask_ptr, mask_idx, query_row)
    et = _idx64(eval_target.reshape(-1), "eval_target")
    rank = torch.empty(n, dtype=torch.int32, device=query_mat.device)
    tsc = torch.empty(n, dtype=torch.float32, device=query_mat.device)
    n_mask_rows = 0 if mask_ptr is None else mask_ptr.numel() - 1
    abi.check(abi.lib().wr_rank_eval_rows(_p(query_mat), query_mat.shape[0], _p(item_tab), item_tab.shape[0], query_mat.shape[1],
                                          _p(qr), _p(et), n, _p(mr), n_mask_rows, _p(mask_ptr), _p(mask_idx), _p(rank), _p(tsc),
                                          _stream()),
              "wr_rank_eval_rows")
    return rank, tsc


RANK_EVAL_MULTI_KQ = (1, 2, 4)


def rank_eval_multi_supports(D, KQ):
    """(embedding size, queries per row) wr_rank_eval_multi takes (wr_rank_eval_multi_supported): rank_eval's D, KQ in {1, 2, 4}"""
    return bool(abi.lib().wr_rank_eval_multi_supported(int(D), int(KQ)))


def rank_eval_multi(queries, item_tab, eval_target, mask_row=None, mask_ptr=None, mask_idx=None):
    """rank_eval_rows for a model with KQ query vectors per row (wr_rank_eval_multi; IF4Rec's interests): queries [n, KQ, D],
    the score of row e against item j is max_k <queries[e, k], item_tab[j]>, and row e is masked by the list of row mask_row[e]
    of the CSR (repeated KQ times here, on the device: the scan sees n KQ query rows).  Returns (rank int32 [n], target_score
    fp32 [n]); with KQ = 1 the bits of rank_eval_rows."""
    _req(queries, torch.float32, "queries", 3)
    n, KQ, D = (int(v) for v in queries.shape)
    if not rank_eval_multi_supports(D, KQ):
        raise abi.WhisprRecHipError("rank_eval_multi does not support D=%d with %d queries per row (D as for rank_eval, queries per "
                                    "row in {1, 2, 4})" % (D, KQ))
    qmat = queries.view(n * KQ, D)
    if eval_target.numel() != n:
        raise ValueError("rank_eval_multi: eval_target has %d entries for %d rows" % (eval_target.numel(), n))
    _, _, mr = _rows_args("rank_eval_multi", qmat, item_tab, n, mask_row, mask_ptr, mask_idx, None)
    et = _idx64(eval_target.reshape(-1), "eval_target")
    if mr is not None:
        mr = mr.repeat_interleave(KQ).contiguous()
    rank = torch.empty(n, dtype=torch.int32, device=queries.device)
    tsc = torch.empty(n, dtype=torch.float32, device=queries.device)
    n_mask_rows = 0 if mask_ptr is None else mask_ptr.numel() - 1
    abi.check(abi.lib().wr_rank_eval_multi(_p(qmat), n * KQ, _p(item_tab), item_tab.shape[0], D, KQ, _p(et), n, _p(mr), n_mask_rows,
                                           _p(mask_ptr), _p(mask_idx), _p(rank), _p(tsc), _stream()),
              "wr_rank_eval_multi")
    return rank, tsc


def topk_recommend_rows(query_mat, item_tab, k, mask_row=None, mask_ptr=None, mask_idx=None, query_row=None):
    """topk_recommend with one query vector per row (wr_topk_recommend_rows; the roles as in rank_eval_rows): n =
    len(query_row), or every row of query_mat.  Order, ties, padding and the bits of the scores are topk_recommend's.
    Returns (items int64 [n, k], scores float32 [n, k]) on the device."""
    n, qr, mr = _rows_args("topk_recommend_rows", query_mat, item_tab, None, mask_row, mask_ptr, mask_idx, query_row)
    k, D = int(k), int(query_mat.shape[1])
    if not topk_supports(D, k):
        raise abi.WhisprRecHipError("topk_recommend_rows does not support D=%d, k=%d (1 <= k <= %d; D as for rank_eval)"
                                    % (D, k, TOPK_MAX_K))
    L, dev = abi.lib(), query_mat.device
    n_items = item_tab.shape[0]
    n_mask_rows = 0 if mask_ptr is None else mask_ptr.numel() - 1
    items = torch.empty((n, k), dtype=torch.int32, device=dev)
    scores = torch.empty((n, k), dtype=torch.float32, device=dev)
    for lo, hi, buf in _topk_blocks(n, n_items, D, k, dev):
        # without query_row a block's queries are the rows lo.. of query_mat: the table pointer moves with the block
        qmat, q_rows = (query_mat, query_mat.shape[0]) if qr is not None else (query_mat[lo:hi], hi - lo)
        abi.check(L.wr_topk_recommend_rows(_p(qmat), q_rows, _p(item_tab), n_items, D, _p(qr[lo:hi]) if qr is not None else None,
                                           hi - lo, _p(mr[lo:hi]) if mr is not None else None, n_mask_rows, _p(mask_ptr),
                                           _p(mask_idx), k, _p(items[lo:hi]), _p(scores[lo:hi]), _p(buf), buf.numel(),
                                           _stream()),
                  "wr_topk_recommend_rows")
    return items.to(torch.int64), scores


def topk_multi_supports(D, KQ, k):
    """(embedding size, queries per row, k) wr_topk_recommend_multi takes (wr_topk_multi_supported): topk_supports' D and k,
    KQ in {1, 2, 4}"""
    return bool(abi.lib().wr_topk_multi_supported(int(D), int(KQ), int(k)))


def topk_recommend_multi(queries, item_tab, k, mask_row=None, mask_ptr=None, mask_idx=None, with_interest=False):
    """topk_recommend_rows for a model with KQ query vectors per row (wr_topk_recommend_multi; IF4Rec's interests): queries
    [n, KQ, D], the score of row e against item j is max_q <queries[e, q], item_tab[j]>, and row e is masked by the list of row
    mask_row[e] of the CSR (repeated KQ times here, on the device, as in rank_eval_multi).  Order, ties and padding are
    topk_recommend's; a score is bitwise rank_eval_multi's target_score of that pair.  Returns (items int64 [n, k], scores
    float32 [n, k]) on the device, and with with_interest=True also interest int64 [n, k]: the smallest q that attains the
    score, -1 at padding."""
    _req(queries, torch.float32, "queries", 3)
    n, KQ, D = (int(v) for v in queries.shape)
    k = int(k)
    if not topk_multi_supports(D, KQ, k):
        raise abi.WhisprRecHipError("topk_recommend_multi does not support D=%d with %d queries per row at k=%d (1 <= k <= %d; D "
                                    "as for rank_eval; queries per row in {1, 2, 4})" % (D, KQ, k, TOPK_MAX_K))
    qmat = queries.view(n * KQ, D)
    _, _, mr = _rows_args("topk_recommend_multi", qmat, item_tab, n, mask_row, mask_ptr, mask_idx, None)
    if mr is not None:
        mr = mr.repeat_interleave(KQ).contiguous()
    L, dev = abi.lib(), queries.device
    n_items = item_tab.shape[0]
    n_mask_rows = 0 if mask_ptr is None else mask_ptr.numel() - 1
    items = torch.empty((n, k), dtype=torch.int32, device=dev)
    scores = torch.empty((n, k), dtype=torch.float32, device=dev)
    interest = torch.empty((n, k), dtype=torch.int32, device=dev) if with_interest else None

    def nbytes(rows):
        return abi.check_size(L.wr_topk_multi_workspace_bytes(rows, n_items, D, KQ, k), "wr_topk_multi_workspace_bytes")

    for lo, hi, buf in _topk_blocks(n, n_items, D, k, dev, nbytes):
        # a block's queries are the rows lo KQ .. of qmat: the table pointer moves with the block
        abi.check(L.wr_topk_recommend_multi(_p(qmat[lo * KQ:hi * KQ]), (hi - lo) * KQ, _p(item_tab), n_items, D, KQ, hi - lo,
                                            _p(mr[lo * KQ:hi * KQ]) if mr is not None else None, n_mask_rows, _p(mask_ptr),
                                            _p(mask_idx), k, _p(items[lo:hi]), _p(scores[lo:hi]),
                                            _p(interest[lo:hi]) if with_interest else None, _p(buf), buf.numel(), _stream()),
                  "wr_topk_recommend_multi")
    if with_interest:
        return items.to(torch.int64), scores, interest.to(torch.int64)
    return items.to(torch.int64), scores


# ----------------------------------------------------------------------------------------------- InfoNCE (SGL)
def infonce_supports(D):
    """embedding sizes wr_infonce_loss_grad takes (wr_infonce_supported)"""
    return bool(abi.lib().wr_infonce_supported(int(D)))


def infonce_workspace_bytes(n, B, D):
    return abi.check_size(abi.lib().wr_infonce_workspace_bytes(int(n), int(B), int(D)), "wr_infonce_workspace_bytes")


def infonce_loss_grad(A, Bm, idx, tau, weight=1.0, *, loss=None, grads=True, validate=True, out=None):
    """One side of SGL's calc_ssl_loss without the [B, n] score matrix (wr_infonce_loss_grad):
    loss = weight * sum_b (log sum_j exp(<q_b, k_j> / tau) - <q_b, k_idx_b> / tau) over the L2-normalised rows q of A[idx]
    and k of Bm, and its gradients w.r.t. A and Bm.  `loss`: a (1,) device tensor to ADD this side's loss to (None = a
    fresh one).  `grads=False`: loss only.  `out=(gA, gB)`: [n, D] tensors (slices of a larger table are fine) to write
    instead of fresh ones.  `validate=False` skips the read-back of the error word (ids already range-checked).
    Returns (loss, gA, gB)."""
    _req(A, torch.float32, "A", 2)
    _req(Bm, torch.float32, "Bm", 2)
    ids = _idx64(idx.reshape(-1), "idx")
    if tuple(A.shape) != tuple(Bm.shape):
        raise ValueError("A and Bm must have the same shape (got %s, %s)" % (tuple(A.shape), tuple(Bm.shape)))
    n, D = int(A.shape[0]), int(A.shape[1])
    B = ids.numel()
    if not infonce_supports(D):
        raise abi.WhisprRecHipError("infonce_loss_grad does not support D=%d (D in {32, 64, 128})" % D)
    _check_tau(tau)
    dev = A.device
    loss, accumulate = _loss_slot(loss, dev)
    gA = gB = None
    if grads:
        if out is not None:
            gA, gB = out
            for t, nm in ((gA, "gA"), (gB, "gB")):
                _req(t, torch.float32, nm, 2)
                if tuple(t.shape) != (n, D):
                    raise ValueError("%s must be [%d, %d]" % (nm, n, D))
        else:
            gA = torch.empty((n, D), dtype=torch.float32, device=dev)
            gB = torch.empty((n, D), dtype=torch.float32, device=dev)
    ws, err = _shape_workspace("infonce", dev, (n, B, D), infonce_workspace_bytes, err_word=True)
    if validate:
        err.zero_()
    abi.check(abi.lib().wr_infonce_loss_grad(_p(A), _p(Bm), n, D, _p(ids), B, float(tau), float(weight), _p(loss),
                                             int(accumulate), _p(gA), _p(gB), _p(err) if validate else None, _p(ws), ws.numel(),
                                             _stream()),
              "wr_infonce_loss_grad")
    if validate and int(err.item()) != 0:
        raise IndexError("infonce_loss_grad: idx holds an id outside [0, %d)" % n)
    return loss, gA, gB


def infonce_release_workspaces():
    """drop the cached workspaces (they are as large as a table at big n)"""
    _release_shape_workspaces("infonce")


# ----------------------------------------------------------------------------------------------- full-catalogue softmax loss (K26)
def softmax_ce_supports(D):
    """embedding sizes wr_softmax_ce_loss_grad takes (wr_softmax_ce_supported)"""
    return bool(abi.lib().wr_softmax_ce_supported(int(D)))


def softmax_ce_workspace_bytes(n, B, D):
    return abi.check_size(abi.lib().wr_softmax_ce_workspace_bytes(int(n), int(B), int(D)), "wr_softmax_ce_workspace_bytes")


def softmax_ce_loss_grad(Q, E, target, *, first_class=1, weight=None, loss=None, grads=True, validate=True, out=None,
                         err_word=None):
    """Softmax cross-entropy of the queries Q [B, D] against the whole item table E [n, D] without the [B, n] logit matrix
    (wr_softmax_ce_loss_grad): loss = weight * sum_b (log sum_{j >= first_class} exp(<Q[b], E[j]>) - <Q[b], E[target_b]>) and its
    gradients w.r.t. Q and E (rows below first_class of gE are zeros).  `weight=None`: 1 / B, the mean.  `loss`: a (1,) device
    tensor to ADD the loss to (None = a fresh one).  `grads=False`: loss only, the same bits.  `out=(gQ, gE)`: tensors to write
    instead of fresh ones.  `validate=False` skips the read-back of the error word (targets already range-checked).
    `err_word`: the caller's own int32 device word instead — a bad target ORs 1 into it (and is clamped); the caller clears and
    reads it, nothing is read back here.  Returns (loss, gQ, gE)."""
    _req(Q, torch.float32, "Q", 2)
    _req(E, torch.float32, "E", 2)
    tg = _idx64(target.reshape(-1), "target")
    B, D = int(Q.shape[0]), int(Q.shape[1])
    n = int(E.shape[0])
    if int(E.shape[1]) != D:
        raise ValueError("Q and E must have one row length (got %s, %s)" % (tuple(Q.shape), tuple(E.shape)))
    if tg.numel() != B:
        raise ValueError("target must name one item per row of Q (got %d for %d rows)" % (tg.numel(), B))
    if not softmax_ce_supports(D):
        raise abi.WhisprRecHipError("softmax_ce_loss_grad does not support D=%d (D in {32, 64, 128})" % D)
    if weight is None:
        weight = 1.0 / B
    dev = Q.device
    loss, accumulate = _loss_slot(loss, dev)
    gQ = gE = None
    if grads:
        if out is not None:
            gQ, gE = out
            for t, nm, rows in ((gQ, "gQ", B), (gE, "gE", n)):
                _req(t, torch.float32, nm, 2)
                if tuple(t.shape) != (rows, D):
                    raise ValueError("%s must be [%d, %d]" % (nm, rows, D))
        else:
            gQ = torch.empty((B, D), dtype=torch.float32, device=dev)
            gE = torch.empty((n, D), dtype=torch.float32, device=dev)
    ws, err = _shape_workspace("softmax_ce", dev, (n, B, D), softmax_ce_workspace_bytes, err_word=True)
    if err_word is not None:
        err, validate = _req(err_word, torch.int32, "err_word"), False
    elif validate:
        err.zero_()
    else:
        err = None
    abi.check(abi.lib().wr_softmax_ce_loss_grad(_p(Q), B, _p(E), n, D, _p(tg), int(first_class), float(weight), _p(loss),
                                                int(accumulate), _p(gQ), _p(gE), _p(err), _p(ws), ws.numel(), _stream()),
              "wr_softmax_ce_loss_grad")
    if validate and int(err.item()) != 0:
        raise IndexError("softmax_ce_loss_grad: target holds an item outside [%d, %d)" % (int(first_class), n))
    return loss, gQ, gE


def softmax_ce_release_workspaces():
    """drop the cached workspaces (they are as large as a few tables at big n)"""
    _release_shape_workspaces("softmax_ce")


class _SoftmaxCe(torch.autograd.Function):
    """loss and both gradients in one call of wr_softmax_ce_loss_grad; the backward scales the stored gradients into NEW tensors
    (a second backward gives the same gradients, not twice-scaled ones)"""

    @staticmethod
    def forward(ctx, Q, E, target, first_class, need, err_word):
        loss, gQ, gE = softmax_ce_loss_grad(Q.detach().contiguous(), E.detach().contiguous(), target, first_class=first_class,
                                            grads=need, err_word=err_word)
        if need:
            ctx.save_for_backward(gQ, gE)
        return loss[0]

    @staticmethod
    def backward(ctx, grad_out):
        gQ, gE = ctx.saved_tensors
        return (gQ * grad_out if ctx.needs_input_grad[0] else None, gE * grad_out if ctx.needs_input_grad[1] else None, None, None,
                None, None)


def softmax_ce_loss(Q, E, target, first_class=1, err_word=None):
    """softmax_ce_loss_grad (mean over the batch) under autograd: a 0-d loss whose backward hands Q and E the kernel's gradients.
    Under torch.no_grad(), or when neither input requires a gradient: loss only.  A target outside [first_class, n) raises
    IndexError, or (`err_word`: an int32 device word the caller clears and reads) ORs 1 into the word with no host round trip."""
    need = torch.is_grad_enabled() and (Q.requires_grad or E.requires_grad)
    return _SoftmaxCe.apply(Q, E, target, int(first_class), need, err_word)


# ----------------------------------------------------------------------------------------------- SASRec block (K13)
SASBLOCK_PARAMS = ("masked_attn_head.q_linear.weight", "masked_attn_head.q_linear.bias", "masked_attn_head.k_linear.weight",
                   "masked_attn_head.k_linear.bias", "masked_attn_head.v_linear.weight", "masked_attn_head.v_linear.bias",
                   "layer_norm1.weight", "layer_norm1.bias", "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias",
                   "layer_norm2.weight", "layer_norm2.bias")           # _Block.state_dict() order = the order of the C-ABI


def sasblock_supports(D, d_ff, n_heads, T):
    """shapes wr_sasblock_fwd / _bwd take (wr_sasblock_supported)"""
    return bool(abi.lib().wr_sasblock_supported(int(D), int(d_ff), int(n_heads), int(T)))


def sasblock_workspace_bytes(B, T, D, d_ff, n_heads):
    return abi.check_size(abi.lib().wr_sasblock_workspace_bytes(int(B), int(T), int(D), int(d_ff), int(n_heads)),
                          "wr_sasblock_workspace_bytes")


def _sasblock_call_args(x, params, n_heads):
    B, T, D = (int(v) for v in x.shape)
    d_ff = int(params[8].shape[0])
    shapes = [(D, D), (D,)] * 3 + [(D,), (D,), (d_ff, D), (d_ff,), (D, d_ff), (D,), (D,), (D,)]
    for t, nm, shp in zip(params, SASBLOCK_PARAMS, shapes):
        _req(t, torch.float32, nm)
        if tuple(t.shape) != shp:
            raise ValueError("%s must be %s (got %s)" % (nm, shp, tuple(t.shape)))
    if not sasblock_supports(D, d_ff, n_heads, T):
        raise abi.WhisprRecHipError("sasrec_block does not support D=%d d_ff=%d n_heads=%d T=%d (D = d_ff in {32, 64}, n_heads in "
                                    "{1, 2, 4} with D / n_heads >= 8, T <= 64)" % (D, d_ff, n_heads, T))
    ptrs = (ctypes.c_void_p * len(params))(*[t.data_ptr() for t in params])
    ws = workspace(x.device, "sasblock").get(sasblock_workspace_bytes(B, T, D, d_ff, n_heads))
    return B, T, D, d_ff, ptrs, ws


class _SasBlock(torch.autograd.Function):
    """wr_sasblock_fwd / wr_sasblock_bwd (key_len None) or their _keys variants: saves x and the call's score maximum, nothing
    else"""

    @staticmethod
    def forward(ctx, x, n_heads, p, seed, training, key_len, err, *params):
        x = _req(x.detach().contiguous(), torch.float32, "x", 3)
        params = [t.detach() for t in params]
        B, T, D, d_ff, ptrs, ws = _sasblock_call_args(x, params, n_heads)
        out = torch.empty_like(x)
        gmax = torch.empty(1, dtype=torch.float32, device=x.device)
        L = abi.lib()
        if key_len is None:
            abi.check(L.wr_sasblock_fwd(_p(x), B, T, D, d_ff, int(n_heads), _addr(ptrs), float(p), int(seed), int(bool(training)),
                                        _p(out), _p(gmax), _p(ws), ws.numel(), _stream()), "wr_sasblock_fwd")
        else:
            abi.check(L.wr_sasblock_fwd_keys(_p(x), B, T, D, d_ff, int(n_heads), _addr(ptrs), float(p), int(seed),
                                             int(bool(training)), _p(out), _p(gmax), _p(ws), ws.numel(), _stream(), _p(key_len),
                                             _p(err)), "wr_sasblock_fwd_keys")
        ctx.save_for_backward(x, gmax, *params)
        ctx.key_len = key_len
        ctx.conf = (int(n_heads), float(p), int(seed), int(bool(training)))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, gmax = ctx.saved_tensors[:2]
        params = list(ctx.saved_tensors[2:])
        n_heads, p, seed, training = ctx.conf
        grad_out = _req(grad_out.contiguous(), torch.float32, "grad_out", 3)
        B, T, D, d_ff, ptrs, ws = _sasblock_call_args(x, params, n_heads)
        gx = torch.empty_like(x)
        packed = torch.empty(sum(t.numel() for t in params), dtype=torch.float32, device=x.device)
        L = abi.lib()
        if ctx.key_len is None:
            abi.check(L.wr_sasblock_bwd(_p(x), _p(grad_out), B, T, D, d_ff, n_heads, _addr(ptrs), p, seed, training, _p(gmax),
                                        _p(gx), _p(packed), _p(ws), ws.numel(), _stream()), "wr_sasblock_bwd")
        else:       # the forward has reported a bad length already
            abi.check(L.wr_sasblock_bwd_keys(_p(x), _p(grad_out), B, T, D, d_ff, n_heads, _addr(ptrs), p, seed, training, _p(gmax),
                                             _p(gx), _p(packed), _p(ws), ws.numel(), _stream(), _p(ctx.key_len), None),
                      "wr_sasblock_bwd_keys")
        views, o = [], 0
        for t in params:                                  # the packed gradient, returned as views
            views.append(packed[o:o + t.numel()].view(t.shape))
            o += t.numel()
        return (gx, None, None, None, None, None, None, *views)


def sasblock_params(block):
    """the 14 parameters of a sasrec._Block in the order of the C-ABI"""
    sd = dict(block.named_parameters())
    return [sd[n] for n in SASBLOCK_PARAMS]


def sasrec_block(x, block_module, n_heads, p, seed, training, key_lengths=None, err_word=None):
    """One whole transformer block of SASRec (sasrec._Block / layers.py:8-86) on x [B, T, D] by the fused HIP kernels, under
    autograd: two launches forward, two backward.  Dropout p is applied iff `training`, with the counter-based mask of
    wr_sasblock.hip keyed by `seed` (not torch's generator); the backward recomputes it.
    key_lengths None: the causal mask.  key_lengths int64 [B] on the device: every query keeps the keys j < key_lengths[b]
    (ContraRec's BERT4RecEncoder); a length outside [1, T] is clamped and ORs 1 into `err_word` (an int32 (1,) device tensor the
    caller clears and reads, or None) — no host round trip here."""
    if key_lengths is not None:
        key_lengths = _idx64(key_lengths.reshape(-1), "key_lengths")
        if key_lengths.numel() != x.shape[0]:
            raise ValueError("key_lengths must hold one length per sequence (got %d for B=%d)" % (key_lengths.numel(), x.shape[0]))
        if err_word is not None:
            _req(err_word, torch.int32, "err_word")
    return _SasBlock.apply(x, int(n_heads), float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, bool(training), key_lengths, err_word,
                           *sasblock_params(block_module))


# ----------------------------------------------------------------------------------------------- supervised contrastive loss (K15)
def supcon_supports(D):
    """embedding sizes wr_supcon_loss_grad takes (wr_supcon_supported)"""
    return bool(abi.lib().wr_supcon_supported(int(D)))


SUPCON_MAX_ROWS = 1 << 15


def supcon_workspace_bytes(B, D):
    return abi.check_size(abi.lib().wr_supcon_workspace_bytes(int(B), int(D)), "wr_supcon_workspace_bytes")


def supcon_loss_grad(F, labels, tau, weight=1.0, *, loss=None, grads=True):
    """ContraRec's supervised contrastive loss (ContraLoss, ContraRec.py:141-204, as written: double shift by the row maximum,
    both + 1e-10) over F [2B, D] — raw, unnormalised; rows 0..B-1 view a, rows B..2B-1 view b, row r labelled labels[r mod B] —
    and its gradient w.r.t. F, without a [2B, 2B] array (wr_supcon_loss_grad).  `loss`: a (1,) device tensor to ADD weight * loss
    to (None = a fresh one).  `grads=False`: loss only, same bits.  Returns (loss, gF)."""
    _req(F, torch.float32, "F", 2)
    lab = _idx64(labels.reshape(-1), "labels")
    N, D = int(F.shape[0]), int(F.shape[1])
    B = lab.numel()
    if N != 2 * B:
        raise ValueError("F must hold 2 * len(labels) rows (got %d rows, %d labels)" % (N, B))
    if not supcon_supports(D) or B < 1 or N > SUPCON_MAX_ROWS:
        raise abi.WhisprRecHipError("supcon_loss_grad does not support D=%d, B=%d (D in {32, 64, 128}, 1 <= B, 2 B <= %d)"
                                    % (D, B, SUPCON_MAX_ROWS))
    _check_tau(tau)
    dev = F.device
    loss, accumulate = _loss_slot(loss, dev)
    gF = torch.empty((N, D), dtype=torch.float32, device=dev) if grads else None
    ws = _shape_workspace("supcon", dev, (B, D), supcon_workspace_bytes)
    abi.check(abi.lib().wr_supcon_loss_grad(_p(F), B, D, _p(lab), float(tau), _p(loss), int(accumulate), float(weight), _p(gF), None,
                                            _p(ws), ws.numel(), _stream()), "wr_supcon_loss_grad")
    return loss, gF


def supcon_release_workspaces():
    """drop the cached workspaces"""
    _release_shape_workspaces("supcon")


class _SupCon(torch.autograd.Function):
    """loss and gradient in one call of wr_supcon_loss_grad; the backward scales the stored gradient"""

    @staticmethod
    def forward(ctx, F, labels, tau):
        loss, gF = supcon_loss_grad(F.detach().contiguous(), labels, tau)
        ctx.save_for_backward(gF)
        return loss[0]

    @staticmethod
    def backward(ctx, grad_out):
        (gF,) = ctx.saved_tensors
        return gF * grad_out, None, None


def supcon_loss(F, labels, tau):
    """supcon_loss_grad under autograd: a 0-d loss whose backward hands F the kernel's gradient"""
    return _SupCon.apply(F, labels, float(tau))


# ----------------------------------------------------------------------------------------------- ContraRec's augmented views (K21)
def seq_augment_supports(T, beta_a, beta_b):
    """shapes wr_seq_augment takes (wr_seq_augment_supported): 1 <= T <= 64, integer beta_a, beta_b >= 1, beta_a + beta_b - 1 <= 15"""
    if int(beta_a) != beta_a or int(beta_b) != beta_b:
        return False
    return bool(abi.lib().wr_seq_augment_supported(int(T), int(beta_a), int(beta_b)))


def seq_augment(hist, lengths, rows, mask_token, beta_a, beta_b, seed, epoch, err_word=None, out=None):
    """ContraRec's two augmented views (ContraRec.py:107-129) of the histories of the dataset rows `rows` [B] (any order, repeats
    allowed) in one launch of wr_seq_augment: hist [n_rows, T] left-aligned and zero-padded, lengths [n_rows] -> (a, b), int64
    [B, T].  The reference's distribution from a counter-based generator keyed by (seed, epoch, row id, view), not NumPy's stream:
    a row's views do not depend on the batch.  A length outside [1, T] is clamped and ORs 1, a row id outside the table gives a
    zero row and ORs 2 into `err_word` (an int32 (1,) device tensor the caller clears and reads, or None).  `out`: a pair of
    [B, T] int64 tensors to write into."""
    _req(hist, torch.int64, "hist", 2)
    _req(lengths, torch.int64, "lengths", 1)
    if not isinstance(rows, torch.Tensor) or rows.dim() != 1:
        raise ValueError("rows must be a [B] tensor")
    rows = _idx64(rows, "rows")
    n_rows, T = (int(v) for v in hist.shape)
    B = rows.numel()
    if lengths.numel() != n_rows:
        raise ValueError("lengths must hold one entry per row of hist (got %d for %d rows)" % (lengths.numel(), n_rows))
    if n_rows < 1 or not seq_augment_supports(T, beta_a, beta_b):
        raise abi.WhisprRecHipError("seq_augment does not support T=%d beta=(%r, %r) n_rows=%d (1 <= T <= 64, integer a, b >= 1, "
                                    "a + b - 1 <= 15, n_rows >= 1)" % (T, beta_a, beta_b, n_rows))
    if err_word is not None:
        _req(err_word, torch.int32, "err_word")
    if out is None:
        out = (torch.empty((B, T), dtype=torch.int64, device=hist.device), torch.empty((B, T), dtype=torch.int64, device=hist.device))
    for t, name in zip(out, ("out[0]", "out[1]")):
        _req(t, torch.int64, name, 2)
        if tuple(t.shape) != (B, T):
            raise ValueError("%s must be [B, T] = %s (got %s)" % (name, (B, T), tuple(t.shape)))
    mask64 = (1 << 64) - 1
    abi.check(abi.lib().wr_seq_augment(_p(hist), _p(lengths), n_rows, T, _p(rows), B, int(mask_token), int(beta_a), int(beta_b),
                                       int(seed) & mask64, int(epoch) & mask64, _p(out[0]), _p(out[1]), _p(err_word), _stream()),
              "wr_seq_augment")
    return out[0], out[1]


# ----------------------------------------------------------------------------------------------- BUIR (K16, K17)
def buir_supports(D):
    """embedding sizes wr_buir_loss_grad takes (wr_buir_supported)"""
    return bool(abi.lib().wr_buir_supported(int(D)))


BUIR_MAX_BATCH = 1 << 22


def buir_workspace_bytes(B, D):
    return abi.check_size(abi.lib().wr_buir_workspace_bytes(int(B), int(D)), "wr_buir_workspace_bytes")


def buir_loss_grad(user_online_w, item_online_w, user_target_w, item_target_w, W, b, users, items, *, grads=True, err_word=None):
    """BUIR's bootstrap loss (BUIR.py:76-97) over the batch (users, items) and every gradient of it, in one call of
    wr_buir_loss_grad.  Returns (loss (1,), gU [B, D], gI [B, D], gW [D, D], gb [D]): gU / gI are PER-SAMPLE gradients w.r.t. the
    gathered online rows, targets are constants.  `grads=False`: loss only (the other four are None), same bits.  An id outside
    its table is clamped and ORs 1 into `err_word` (an int32 (1,) device tensor the caller clears and reads, or None)."""
    for t, nm in ((user_online_w, "user_online_w"), (item_online_w, "item_online_w"), (user_target_w, "user_target_w"),
                  (item_target_w, "item_target_w"), (W, "W")):
        _req(t, torch.float32, nm, 2)
    _req(b, torch.float32, "b", 1)
    uu, ii = _idx64(users.reshape(-1), "users"), _idx64(items.reshape(-1), "items")
    B, D = uu.numel(), int(W.shape[0])
    if ii.numel() != B:
        raise ValueError("users and items must hold one id per sample (got %d and %d)" % (B, ii.numel()))
    if user_target_w.shape != user_online_w.shape or item_target_w.shape != item_online_w.shape:
        raise ValueError("a target table must have the shape of its online table")
    if tuple(W.shape) != (D, D) or b.numel() != D or user_online_w.shape[1] != D or item_online_w.shape[1] != D:
        raise ValueError("W must be [D, D] and b [D] with D the embedding size of the tables")
    if not buir_supports(D) or B < 1 or B > BUIR_MAX_BATCH:
        raise abi.WhisprRecHipError("buir_loss_grad does not support D=%d, B=%d (D in {32, 64, 128}, 1 <= B <= %d)"
                                    % (D, B, BUIR_MAX_BATCH))
    if err_word is not None:
        _req(err_word, torch.int32, "err_word")
    dev = W.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    gU = gI = gW = gb = None
    if grads:
        gU = torch.empty((B, D), dtype=torch.float32, device=dev)
        gI = torch.empty((B, D), dtype=torch.float32, device=dev)
        gW = torch.empty((D, D), dtype=torch.float32, device=dev)
        gb = torch.empty(D, dtype=torch.float32, device=dev)
    ws = _shape_workspace("buir", dev, (B, D), buir_workspace_bytes)
    abi.check(abi.lib().wr_buir_loss_grad(_p(user_online_w), _p(item_online_w), _p(user_target_w), _p(item_target_w),
                                          user_online_w.shape[0], item_online_w.shape[0], D, _p(W), _p(b), _p(uu), _p(ii), B, _p(loss),
                                          _p(gU), _p(gI), _p(gW), _p(gb), _p(err_word), _p(ws), ws.numel(), _stream()),
              "wr_buir_loss_grad")
    return loss, gU, gI, gW, gb


def buir_release_workspaces():
    """drop the cached workspaces"""
    _release_shape_workspaces("buir")


class _BuirLoss(torch.autograd.Function):
    """loss and gradients in one call of wr_buir_loss_grad; the backward scales the stored gradients into NEW tensors (a second
    backward gives the same gradients) and scatter-adds the per-sample rows into dense table gradients"""

    @staticmethod
    def forward(ctx, user_online_w, item_online_w, W, b, user_target_w, item_target_w, users, items, err_word, need):
        loss, gU, gI, gW, gb = buir_loss_grad(user_online_w.detach(), item_online_w.detach(), user_target_w.detach(),
                                              item_target_w.detach(), W.detach(), b.detach(), users, items, grads=need,
                                              err_word=err_word)
        if need:
            # the kernel read clamped ids; the scatter below must not leave the tables either
            uu = users.reshape(-1).clamp(0, user_online_w.shape[0] - 1)
            ii = items.reshape(-1).clamp(0, item_online_w.shape[0] - 1)
            ctx.save_for_backward(gU, gI, gW, gb, uu, ii)
            ctx.shapes = (tuple(user_online_w.shape), tuple(item_online_w.shape))
        return loss[0]

    @staticmethod
    def backward(ctx, grad_out):
        gU, gI, gW, gb, uu, ii = ctx.saved_tensors
        su, si = ctx.shapes
        dU = scatter_add_rows(torch.zeros(su, dtype=torch.float32, device=gU.device), uu, gU * grad_out)
        dI = scatter_add_rows(torch.zeros(si, dtype=torch.float32, device=gI.device), ii, gI * grad_out)
        return dU, dI, gW * grad_out, gb * grad_out, None, None, None, None, None, None


def buir_loss(user_online_w, item_online_w, user_target_w, item_target_w, W, b, users, items, err_word=None):
    """buir_loss_grad under autograd: a 0-d loss whose backward hands the two online tables dense gradients (scatter_add_rows of
    the per-sample rows) and the predictor its own.  Under torch.no_grad(), or when nothing requires a gradient: loss only."""
    need = torch.is_grad_enabled() and any(t.requires_grad for t in (user_online_w, item_online_w, W, b))
    return _BuirLoss.apply(user_online_w, item_online_w, W, b, user_target_w, item_target_w, users, items, err_word, need)


def ema_update_(target, online, momentum):
    """target = target * momentum + online * (1. - momentum), in place and in one pass (wr_ema_update): the three roundings of
    BUIR._update_target (BUIR.py:71), 1 - momentum formed in double as Python forms it.  Returns target."""
    _req(target, torch.float32, "target")
    _req(online, torch.float32, "online")
    if target.shape != online.shape:
        raise ValueError("target and online must have one shape (got %s and %s)" % (tuple(target.shape), tuple(online.shape)))
    if target.numel():
        abi.check(abi.lib().wr_ema_update(_p(target), _p(online), target.numel(), float(momentum), float(1. - float(momentum)),
                                          _stream()), "wr_ema_update")
    return target


# ----------------------------------------------------------------------------------------------- optimizers
# ----------------------------------------------------------------------------------------------- IF4Rec interest pooling (K18)
def interest_pool_supports(D, A, K, T):
    """shapes wr_interest_pool_fwd / _bwd take (wr_interest_pool_supported): D in {32, 64, 128}, A <= 32, K <= 8, T <= 64"""
    return bool(abi.lib().wr_interest_pool_supported(int(D), int(A), int(K), int(T)))


def interest_pool_workspace_bytes(B, D, A, K, T):
    return abi.check_size(abi.lib().wr_interest_pool_workspace_bytes(int(B), int(D), int(A), int(K), int(T)),
                          "wr_interest_pool_workspace_bytes")


def _interest_pool_args(item_weight, pos_weight, history, W1, b1, W2, b2, err_word):
    """the argument checks of interest_pool_fwd / _bwd -> (history int64 [B, T], B, T, D, A, K)"""
    _req(item_weight, torch.float32, "item_weight", 2)
    if pos_weight is not None:
        _req(pos_weight, torch.float32, "pos_weight", 2)
    _req(W1, torch.float32, "W1", 2)
    _req(b1, torch.float32, "b1", 1)
    _req(W2, torch.float32, "W2", 2)
    _req(b2, torch.float32, "b2", 1)
    if not isinstance(history, torch.Tensor) or history.dim() != 2:
        raise ValueError("history must be a [B, T] tensor")
    hist = _idx64(history, "history")
    B, T = (int(v) for v in hist.shape)
    D, A, K = int(item_weight.shape[1]), int(W1.shape[0]), int(W2.shape[0])
    if tuple(W1.shape) != (A, D) or b1.numel() != A or tuple(W2.shape) != (K, A) or b2.numel() != K:
        raise ValueError("W1 must be [A, D], b1 [A], W2 [K, A] and b2 [K] with D the embedding size of the item table (got %s, %s, "
                         "%s, %s for D=%d)" % (tuple(W1.shape), tuple(b1.shape), tuple(W2.shape), tuple(b2.shape), D))
    if pos_weight is not None and (pos_weight.shape[1] != D or pos_weight.shape[0] < T):
        raise ValueError("pos_weight must hold at least T=%d rows of D=%d (got %s)" % (T, D, tuple(pos_weight.shape)))
    if B < 1 or not interest_pool_supports(D, A, K, T):
        raise abi.WhisprRecHipError("interest_pool does not support B=%d D=%d A=%d K=%d T=%d (D in {32, 64, 128}, 1 <= A <= 32, "
                                    "1 <= K <= 8, 1 <= T <= 64, B >= 1)" % (B, D, A, K, T))
    if err_word is not None:
        _req(err_word, torch.int32, "err_word")
    return hist, B, T, D, A, K


def interest_pool_fwd(item_weight, pos_weight, history, W1, b1, W2, b2, err_word=None):
    """IF4Rec's interest vectors [B, K, D] (IF4Rec.py:87-103) in one launch of wr_interest_pool_fwd: no [B, T, D] gather, no
    [B, K, T, D] product.  pos_weight None: add_pos 0.  An id outside the item table is clamped and ORs 1 into `err_word` (an
    int32 (1,) device tensor the caller clears and reads, or None)."""
    hist, B, T, D, A, K = _interest_pool_args(item_weight, pos_weight, history, W1, b1, W2, b2, err_word)
    out = torch.empty((B, K, D), dtype=torch.float32, device=item_weight.device)
    n_pos = 0 if pos_weight is None else pos_weight.shape[0]
    abi.check(abi.lib().wr_interest_pool_fwd(_p(item_weight), item_weight.shape[0], _p(pos_weight), n_pos, D, _p(hist), B, T, _p(W1),
                                             _p(b1), _p(W2), _p(b2), A, K, _p(out), _p(err_word), _stream()), "wr_interest_pool_fwd")
    return out


def interest_pool_bwd(item_weight, pos_weight, history, W1, b1, W2, b2, g_out, err_word=None):
    """The gradients of interest_pool_fwd for g_out [B, K, D] (wr_interest_pool_bwd; the forward is recomputed from the ids):
    (g_hp [B, T, D], gW1, gb1, gW2, gb2, gpos or None).  g_hp is the gradient w.r.t. item row + position row, exactly 0 at
    masked positions; gpos has the shape of pos_weight.  No float atomics: same inputs, same bits."""
    hist, B, T, D, A, K = _interest_pool_args(item_weight, pos_weight, history, W1, b1, W2, b2, err_word)
    _req(g_out, torch.float32, "g_out", 3)
    if tuple(g_out.shape) != (B, K, D):
        raise ValueError("g_out must be [B, K, D] = %s (got %s)" % ((B, K, D), tuple(g_out.shape)))
    dev = item_weight.device
    g_hp = torch.empty((B, T, D), dtype=torch.float32, device=dev)
    gW1, gb1, gW2, gb2 = (torch.empty_like(t) for t in (W1, b1, W2, b2))
    gpos = None if pos_weight is None else torch.empty_like(pos_weight)
    n_pos = 0 if pos_weight is None else pos_weight.shape[0]
    ws = workspace(dev, "interest_pool").get(interest_pool_workspace_bytes(B, D, A, K, T))
    abi.check(abi.lib().wr_interest_pool_bwd(_p(item_weight), item_weight.shape[0], _p(pos_weight), n_pos, D, _p(hist), B, T, _p(W1),
                                             _p(b1), _p(W2), _p(b2), A, K, _p(g_out), _p(g_hp), _p(gW1), _p(gb1), _p(gW2), _p(gb2),
                                             _p(gpos), _p(err_word), _p(ws), ws.numel(), _stream()), "wr_interest_pool_bwd")
    return g_hp, gW1, gb1, gW2, gb2, gpos


class _InterestPool(torch.autograd.Function):
    """wr_interest_pool_fwd / _bwd: saves the ids and the parameters, no activation"""

    @staticmethod
    def forward(ctx, item_weight, pos_weight, W1, b1, W2, b2, history, err_word):
        args = [t.detach() if t is not None else None for t in (item_weight, pos_weight, W1, b1, W2, b2)]
        out = interest_pool_fwd(args[0], args[1], history, *args[2:], err_word=err_word)
        ctx.has_pos = pos_weight is not None
        ctx.save_for_backward(history, *[t for t in args if t is not None])
        return out

    @staticmethod
    def backward(ctx, grad_out):
        history, item_weight = ctx.saved_tensors[:2]
        rest = list(ctx.saved_tensors[2:])
        pos_weight = rest.pop(0) if ctx.has_pos else None
        W1, b1, W2, b2 = rest
        g_hp, gW1, gb1, gW2, gb2, gpos = interest_pool_bwd(item_weight, pos_weight, history, W1, b1, W2, b2, grad_out.contiguous())
        # the kernel read clamped ids; the scatter must not leave the table either.  Row 0 is the padding id: its rows of g_hp
        # are zeros and are skipped
        g_item = torch.zeros_like(item_weight)
        ids = history.reshape(-1).clamp(0, item_weight.shape[0] - 1)
        scatter_add_rows(g_item, ids, g_hp.view(-1, g_hp.shape[2]), padding_idx=0)
        return g_item, gpos, gW1, gb1, gW2, gb2, None, None


def interest_pool(item_weight, pos_weight, history, W1, b1, W2, b2, err_word=None):
    """interest_pool_fwd under autograd: [B, K, D] whose backward hands back the kernel's gradients of all six parameters (the
    item table's through scatter_add_rows of g_hp, sorted and deterministic)."""
    return _InterestPool.apply(item_weight, pos_weight, W1, b1, W2, b2, history, err_word)


# ----------------------------------------------------------------------------------------------- time-interval attention (K25)
def ti_attention_supports(D, n_heads, T, time_max):
    """shapes wr_ti_attention_fwd / _bwd take (wr_ti_attention_supported): D in {32, 64}, n_heads in {1, 2, 4} with D / n_heads
    >= 8, T <= 64, time_max <= 2048"""
    return bool(abi.lib().wr_ti_attention_supported(int(D), int(n_heads), int(T), int(time_max)))


def ti_attention_workspace_bytes(B, T, D, n_heads, time_max):
    return abi.check_size(abi.lib().wr_ti_attention_workspace_bytes(int(B), int(T), int(D), int(n_heads), int(time_max)),
                          "wr_ti_attention_workspace_bytes")


def _ti_attention_args(q, k, v, times, min_interval, time_k, time_v, n_heads, time_max, err_word):
    """the argument checks of ti_attention_fwd / _bwd -> (B, T, D)"""
    _req(q, torch.float32, "q", 3)
    _req(k, torch.float32, "k", 3)
    _req(v, torch.float32, "v", 3)
    _req(times, torch.int64, "times", 2)
    _req(min_interval, torch.int64, "min_interval", 1)
    _req(time_k, torch.float32, "time_k", 2)
    _req(time_v, torch.float32, "time_v", 2)
    B, T, D = (int(x) for x in q.shape)
    if k.shape != q.shape or v.shape != q.shape or tuple(times.shape) != (B, T) or min_interval.numel() != B:
        raise ValueError("q, k, v must share one shape [B, T, D], times be [B, T] and min_interval [B] (got %s, %s, %s, %s, %s)"
                         % (tuple(q.shape), tuple(k.shape), tuple(v.shape), tuple(times.shape), tuple(min_interval.shape)))
    rows = int(time_max) + 1
    if tuple(time_k.shape) != (rows, D) or tuple(time_v.shape) != (rows, D):
        raise ValueError("time_k and time_v must be [time_max + 1, D] = %s (got %s and %s)"
                         % ((rows, D), tuple(time_k.shape), tuple(time_v.shape)))
    if B < 1 or D % int(n_heads) or not ti_attention_supports(D, n_heads, T, time_max):
        raise abi.WhisprRecHipError("ti_attention does not support B=%d T=%d D=%d n_heads=%d time_max=%d (D in {32, 64}, n_heads in "
                                    "{1, 2, 4} with D / n_heads >= 8, 1 <= T <= 64, 1 <= time_max <= 2048, B >= 1)"
                                    % (B, T, D, int(n_heads), int(time_max)))
    if err_word is not None:
        _req(err_word, torch.int32, "err_word")
    return B, T, D


def ti_attention_fwd(q, k, v, times, min_interval, time_k, time_v, n_heads, time_max, err_word=None):
    """Time-interval attention [B, T, D] (layers.py:105-146 after the projections) in one launch of wr_ti_attention_fwd: the
    intervals min(|t_i - t_j| // m_b, time_max) are formed in the kernel and the table rows looked up while the scores are; no
    [B, T, T, D] gather.  min_interval < 1 is clamped to 1 and ORs 1 into `err_word` (an int32 (1,) device tensor the caller clears
    and reads, or None)."""
    B, T, D = _ti_attention_args(q, k, v, times, min_interval, time_k, time_v, n_heads, time_max, err_word)
    out = torch.empty_like(q)
    abi.check(abi.lib().wr_ti_attention_fwd(_p(q), _p(k), _p(v), _p(times), _p(min_interval), B, T, D, int(n_heads), _p(time_k),
                                            _p(time_v), int(time_max), _p(out), _p(err_word), _stream()), "wr_ti_attention_fwd")
    return out


def ti_attention_bwd(q, k, v, times, min_interval, time_k, time_v, n_heads, time_max, g_out, err_word=None):
    """The gradients of ti_attention_fwd for g_out [B, T, D] (wr_ti_attention_bwd, two launches; the forward is recomputed):
    (gq, gk, gv, g_time_k, g_time_v).  No float atomics: same inputs, same bits."""
    B, T, D = _ti_attention_args(q, k, v, times, min_interval, time_k, time_v, n_heads, time_max, err_word)
    _req(g_out, torch.float32, "g_out", 3)
    if g_out.shape != q.shape:
        raise ValueError("g_out must be [B, T, D] = %s (got %s)" % (tuple(q.shape), tuple(g_out.shape)))
    gq, gk, gv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
    g_tk, g_tv = torch.empty_like(time_k), torch.empty_like(time_v)
    ws = workspace(q.device, "ti_attention").get(ti_attention_workspace_bytes(B, T, D, n_heads, time_max))
    abi.check(abi.lib().wr_ti_attention_bwd(_p(q), _p(k), _p(v), _p(times), _p(min_interval), B, T, D, int(n_heads), _p(time_k),
                                            _p(time_v), int(time_max), _p(g_out), _p(gq), _p(gk), _p(gv), _p(g_tk), _p(g_tv),
                                            _p(err_word), _p(ws), ws.numel(), _stream()), "wr_ti_attention_bwd")
    return gq, gk, gv, g_tk, g_tv


class _TiAttention(torch.autograd.Function):
    """wr_ti_attention_fwd / _bwd: saves the inputs, no activation"""

    @staticmethod
    def forward(ctx, q, k, v, time_k, time_v, times, min_interval, n_heads, time_max, err_word):
        args = [t.detach().contiguous() for t in (q, k, v, time_k, time_v)]
        out = ti_attention_fwd(args[0], args[1], args[2], times, min_interval, args[3], args[4], n_heads, time_max, err_word)
        ctx.n_heads, ctx.time_max = int(n_heads), int(time_max)
        ctx.save_for_backward(times, min_interval, *args)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        times, min_interval, q, k, v, time_k, time_v = ctx.saved_tensors
        gq, gk, gv, g_tk, g_tv = ti_attention_bwd(q, k, v, times, min_interval, time_k, time_v, ctx.n_heads, ctx.time_max,
                                                  grad_out.contiguous())
        return gq, gk, gv, g_tk, g_tv, None, None, None, None, None


def ti_attention(q, k, v, times, min_interval, time_k, time_v, n_heads, time_max, err_word=None):
    """ti_attention_fwd under autograd: [B, T, D] whose backward hands back the kernel's gradients of q, k, v and both tables."""
    return _TiAttention.apply(q, k, v, time_k, time_v, times, min_interval, n_heads, time_max, err_word)


# --------------------------------------------------------------------------------------------------------------- GRU (K27)
def gru_supports(E, H, T):
    """shapes wr_gru_fwd / _bwd take (wr_gru_supported): E, H in {32, 64} in any combination, T >= 1"""
    return bool(abi.lib().wr_gru_supported(int(E), int(H), int(T)))


def gru_workspace_bytes(B, T, E, H):
    return abi.check_size(abi.lib().wr_gru_workspace_bytes(int(B), int(T), int(E), int(H)), "wr_gru_workspace_bytes")


def _gru_args(x, lengths, w_ih, w_hh, b_ih, b_hh):
    """the argument checks of gru_fwd / gru_bwd -> (B, T, E, H)"""
    _req(x, torch.float32, "x", 3)
    _req(lengths, torch.int64, "lengths", 1)
    _req(w_ih, torch.float32, "w_ih", 2)
    _req(w_hh, torch.float32, "w_hh", 2)
    _req(b_ih, torch.float32, "b_ih", 1)
    _req(b_hh, torch.float32, "b_hh", 1)
    B, T, E = (int(s) for s in x.shape)
    H = int(w_hh.shape[1])
    if (lengths.numel() != B or tuple(w_ih.shape) != (3 * H, E) or tuple(w_hh.shape) != (3 * H, H) or b_ih.numel() != 3 * H
            or b_hh.numel() != 3 * H):
        raise ValueError("x must be [B, T, E], lengths [B], w_ih [3H, E], w_hh [3H, H], b_ih and b_hh [3H] (got %s, %s, %s, %s, %s, %s)"
                         % tuple(tuple(t.shape) for t in (x, lengths, w_ih, w_hh, b_ih, b_hh)))
    if B < 1 or not gru_supports(E, H, T):
        raise abi.WhisprRecHipError("gru does not support B=%d T=%d E=%d H=%d (E, H in {32, 64}, T >= 1, B >= 1)" % (B, T, E, H))
    return B, T, E, H


def gru_fwd(x, lengths, w_ih, w_hh, b_ih, b_hh, save_hs=False):
    """One-layer GRU (torch's cell, gates r, z, n, h_0 = 0) over left-aligned histories x [B, T, E] in one launch of wr_gru_fwd ->
    (h_last [B, H], hs): row b takes its first clamp(lengths[b], 0, T) steps, h_last[b] is its state after them (zeros for a
    length of 0); x[b, t, :] is never read at t >= lengths[b].  save_hs: every step's state is also stored, hs [B, T, H] (what
    gru_bwd reads); otherwise hs is None and nothing but h_last is allocated or written."""
    B, T, E, H = _gru_args(x, lengths, w_ih, w_hh, b_ih, b_hh)
    h_last = torch.empty((B, H), dtype=torch.float32, device=x.device)
    hs = torch.empty((B, T, H), dtype=torch.float32, device=x.device) if save_hs else None
    abi.check(abi.lib().wr_gru_fwd(_p(x), _p(lengths), _p(w_ih), _p(w_hh), _p(b_ih), _p(b_hh), B, T, E, H, _p(h_last), _p(hs),
                                   _stream()), "wr_gru_fwd")
    return h_last, hs


def gru_bwd(x, lengths, w_ih, w_hh, b_ih, b_hh, hs, g_last):
    """The gradients of gru_fwd's h_last for g_last [B, H] (wr_gru_bwd, two launches; the gates are recomputed from x and hs):
    (gx [B, T, E], g_w_ih, g_w_hh, g_b_ih, g_b_hh).  gx is exactly zero at t >= lengths[b].  No float atomics: same inputs, same
    bits."""
    B, T, E, H = _gru_args(x, lengths, w_ih, w_hh, b_ih, b_hh)
    _req(hs, torch.float32, "hs", 3)
    _req(g_last, torch.float32, "g_last", 2)
    if tuple(hs.shape) != (B, T, H) or tuple(g_last.shape) != (B, H):
        raise ValueError("hs must be [B, T, H] = %s and g_last [B, H] (got %s and %s)"
                         % ((B, T, H), tuple(hs.shape), tuple(g_last.shape)))
    gx = torch.empty_like(x)
    g_w_ih, g_w_hh, g_b_ih, g_b_hh = (torch.empty_like(t) for t in (w_ih, w_hh, b_ih, b_hh))
    ws = workspace(x.device, "gru").get(gru_workspace_bytes(B, T, E, H))
    abi.check(abi.lib().wr_gru_bwd(_p(x), _p(lengths), _p(w_ih), _p(w_hh), _p(b_ih), _p(b_hh), _p(hs), _p(g_last), B, T, E, H,
                                   _p(gx), _p(g_w_ih), _p(g_w_hh), _p(g_b_ih), _p(g_b_hh), _p(ws), ws.numel(), _stream()),
              "wr_gru_bwd")
    return gx, g_w_ih, g_w_hh, g_b_ih, g_b_hh


gru_stats = {"calls": 0, "hs_bytes": 0}      # of the last gru_last call: the bytes of the step states it kept (0: none)


class _GruLast(torch.autograd.Function):
    """wr_gru_fwd / _bwd: saves the inputs and hs [B, T, H], the one activation"""

    @staticmethod
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh, lengths, save_hs):
        args = [t.detach().contiguous() for t in (x, w_ih, w_hh, b_ih, b_hh)]
        h_last, hs = gru_fwd(args[0], lengths, *args[1:], save_hs=save_hs)
        gru_stats["calls"] += 1
        gru_stats["hs_bytes"] = 0 if hs is None else hs.numel() * hs.element_size()
        if hs is not None:
            ctx.save_for_backward(lengths, hs, *args)
        return h_last

    @staticmethod
    def backward(ctx, g_last):
        lengths, hs, x, w_ih, w_hh, b_ih, b_hh = ctx.saved_tensors
        gx, g_w_ih, g_w_hh, g_b_ih, g_b_hh = gru_bwd(x, lengths, w_ih, w_hh, b_ih, b_hh, hs, g_last.contiguous())
        return gx, g_w_ih, g_w_hh, g_b_ih, g_b_hh, None, None


def gru_last(x, lengths, w_ih, w_hh, b_ih, b_hh):
    """gru_fwd under autograd: h_last [B, H] whose backward hands back the kernel's gx and the four parameter gradients.  Under
    torch.no_grad(), or when neither x nor a parameter requires grad, no step state is kept (gru_stats["hs_bytes"] == 0)."""
    lengths = _idx64(lengths, "lengths")
    save_hs = torch.is_grad_enabled() and any(t.requires_grad for t in (x, w_ih, w_hh, b_ih, b_hh))
    return _GruLast.apply(x, w_ih, w_hh, b_ih, b_hh, lengths, save_hs)


def gru_seq_fwd(x, lengths, w_ih, w_hh, b_ih, b_hh):
    """The same GRU walk in one launch of wr_gru_seq_fwd -> hs [B, T, H], every step's state: row b's first clamp(lengths[b], 0,
    T) steps and EXACTLY ZERO after them (pad_packed_sequence's form; gru_fwd(save_hs=True) stores the frozen state there).
    x[b, t, :] is never read at t >= lengths[b].  For t < lengths[b] the bits are gru_fwd's."""
    B, T, E, H = _gru_args(x, lengths, w_ih, w_hh, b_ih, b_hh)
    hs = torch.empty((B, T, H), dtype=torch.float32, device=x.device)
    abi.check(abi.lib().wr_gru_seq_fwd(_p(x), _p(lengths), _p(w_ih), _p(w_hh), _p(b_ih), _p(b_hh), B, T, E, H, _p(hs), _stream()),
              "wr_gru_seq_fwd")
    return hs


def gru_seq_bwd(x, lengths, w_ih, w_hh, b_ih, b_hh, hs, g_hs, g_last=None):
    """The gradients of gru_seq_fwd's hs for g_hs [B, T, H], which enters at every step t < lengths[b] (its padding is never
    read), and optionally g_last [B, H] on the state after step lengths[b] - 1 (wr_gru_seq_bwd, two launches):
    (gx [B, T, E], g_w_ih, g_w_hh, g_b_ih, g_b_hh).  gx is exactly zero at t >= lengths[b].  Same inputs, same bits."""
    B, T, E, H = _gru_args(x, lengths, w_ih, w_hh, b_ih, b_hh)
    _req(hs, torch.float32, "hs", 3)
    _req(g_hs, torch.float32, "g_hs", 3)
    if g_last is not None:
        _req(g_last, torch.float32, "g_last", 2)
    if tuple(hs.shape) != (B, T, H) or tuple(g_hs.shape) != (B, T, H) or (g_last is not None and tuple(g_last.shape) != (B, H)):
        raise ValueError("hs and g_hs must be [B, T, H] = %s and g_last [B, H] or None (got %s, %s and %s)"
                         % ((B, T, H), tuple(hs.shape), tuple(g_hs.shape), None if g_last is None else tuple(g_last.shape)))
    gx = torch.empty_like(x)
    g_w_ih, g_w_hh, g_b_ih, g_b_hh = (torch.empty_like(t) for t in (w_ih, w_hh, b_ih, b_hh))
    ws = workspace(x.device, "gru").get(gru_workspace_bytes(B, T, E, H))
    abi.check(abi.lib().wr_gru_seq_bwd(_p(x), _p(lengths), _p(w_ih), _p(w_hh), _p(b_ih), _p(b_hh), _p(hs), _p(g_hs), _p(g_last), B,
                                       T, E, H, _p(gx), _p(g_w_ih), _p(g_w_hh), _p(g_b_ih), _p(g_b_hh), _p(ws), ws.numel(),
                                       _stream()), "wr_gru_seq_bwd")
    return gx, g_w_ih, g_w_hh, g_b_ih, g_b_hh


class _GruSeq(torch.autograd.Function):
    """wr_gru_seq_fwd / _bwd: saves the inputs and its own result hs"""

    @staticmethod
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh, lengths):
        args = [t.detach().contiguous() for t in (x, w_ih, w_hh, b_ih, b_hh)]
        hs = gru_seq_fwd(args[0], lengths, *args[1:])
        ctx.save_for_backward(lengths, hs, *args)
        return hs

    @staticmethod
    def backward(ctx, g_hs):
        lengths, hs, x, w_ih, w_hh, b_ih, b_hh = ctx.saved_tensors
        gx, g_w_ih, g_w_hh, g_b_ih, g_b_hh = gru_seq_bwd(x, lengths, w_ih, w_hh, b_ih, b_hh, hs, g_hs.contiguous())
        return gx, g_w_ih, g_w_hh, g_b_ih, g_b_hh, None


def gru_seq(x, lengths, w_ih, w_hh, b_ih, b_hh):
    """gru_seq_fwd under autograd: hs [B, T, H], zero past each row's length, whose backward hands back the kernel's gx and the
    four parameter gradients for a gradient at every step."""
    return _GruSeq.apply(x, w_ih, w_hh, b_ih, b_hh, _idx64(lengths, "lengths"))


# --------------------------------------------------------------------------------------------------------------- NARM pooling (K28)
def narm_pool_supports(H, A, T):
    """shapes wr_narm_pool_fwd / _bwd take (wr_narm_pool_supported): H in {32, 64}, A in {16, 32, 64}, T >= 1"""
    return bool(abi.lib().wr_narm_pool_supported(int(H), int(A), int(T)))


def narm_pool_workspace_bytes(B, T, H, A):
    return abi.check_size(abi.lib().wr_narm_pool_workspace_bytes(int(B), int(T), int(H), int(A)), "wr_narm_pool_workspace_bytes")


def _narm_args(hs, h_g, lengths, A1, A2, v):
    """the argument checks of narm_pool_fwd / _bwd -> (B, T, H, A)"""
    _req(hs, torch.float32, "hs", 3)
    _req(h_g, torch.float32, "h_g", 2)
    _req(lengths, torch.int64, "lengths", 1)
    _req(A1, torch.float32, "A1", 2)
    _req(A2, torch.float32, "A2", 2)
    _req(v, torch.float32, "v", 1)
    B, T, H = (int(s) for s in hs.shape)
    A = int(A1.shape[0])
    if tuple(h_g.shape) != (B, H) or lengths.numel() != B or tuple(A1.shape) != (A, H) or tuple(A2.shape) != (A, H) or v.numel() != A:
        raise ValueError("hs must be [B, T, H], h_g [B, H], lengths [B], A1 and A2 [A, H], v [A] (got %s, %s, %s, %s, %s, %s)"
                         % tuple(tuple(t.shape) for t in (hs, h_g, lengths, A1, A2, v)))
    if B < 1 or not narm_pool_supports(H, A, T):
        raise abi.WhisprRecHipError("narm_pool does not support B=%d T=%d H=%d A=%d (H in {32, 64}, A in {16, 32, 64}, T >= 1, "
                                    "B >= 1)" % (B, T, H, A))
    return B, T, H, A


def narm_pool_fwd(hs, h_g, lengths, A1, A2, v):
    """NARM's attention pooling in one launch of wr_narm_pool_fwd -> c [B, H]: c[b] = sum_{t < len_b} e_t hs[b, t] with
    e_t = v . sigmoid(A1 h_g[b] + A2 hs[b, t]) and len_b = clamp(lengths[b], 0, T); hs[b, t, :] is never read at t >= len_b."""
    B, T, H, A = _narm_args(hs, h_g, lengths, A1, A2, v)
    c = torch.empty((B, H), dtype=torch.float32, device=hs.device)
    abi.check(abi.lib().wr_narm_pool_fwd(_p(hs), _p(h_g), _p(lengths), _p(A1), _p(A2), _p(v), B, T, H, A, _p(c), _stream()),
              "wr_narm_pool_fwd")
    return c


def narm_pool_bwd(hs, h_g, lengths, A1, A2, v, g_c):
    """The gradients of narm_pool_fwd's c for g_c [B, H] (wr_narm_pool_bwd, two launches; sigmoid(u_t) is recomputed):
    (g_hs [B, T, H], g_h_g [B, H], g_A1, g_A2 [A, H], g_v [A]).  g_hs is exactly zero at t >= lengths[b].  Same inputs, same bits."""
    B, T, H, A = _narm_args(hs, h_g, lengths, A1, A2, v)
    _req(g_c, torch.float32, "g_c", 2)
    if tuple(g_c.shape) != (B, H):
        raise ValueError("g_c must be [B, H] = %s (got %s)" % ((B, H), tuple(g_c.shape)))
    g_hs, g_h_g = torch.empty_like(hs), torch.empty_like(h_g)
    g_A1, g_A2, g_v = (torch.empty_like(t) for t in (A1, A2, v))
    ws = workspace(hs.device, "narm").get(narm_pool_workspace_bytes(B, T, H, A))
    abi.check(abi.lib().wr_narm_pool_bwd(_p(hs), _p(h_g), _p(lengths), _p(A1), _p(A2), _p(v), _p(g_c), B, T, H, A, _p(g_hs),
                                         _p(g_h_g), _p(g_A1), _p(g_A2), _p(g_v), _p(ws), ws.numel(), _stream()), "wr_narm_pool_bwd")
    return g_hs, g_h_g, g_A1, g_A2, g_v


class _NarmPool(torch.autograd.Function):
    """wr_narm_pool_fwd / _bwd: saves nothing but the inputs"""

    @staticmethod
    def forward(ctx, hs, h_g, A1, A2, v, lengths):
        args = [t.detach().contiguous() for t in (hs, h_g, A1, A2, v)]
        c = narm_pool_fwd(args[0], args[1], lengths, *args[2:])
        ctx.save_for_backward(lengths, *args)
        return c

    @staticmethod
    def backward(ctx, g_c):
        lengths, hs, h_g, A1, A2, v = ctx.saved_tensors
        return narm_pool_bwd(hs, h_g, lengths, A1, A2, v, g_c.contiguous()) + (None,)


def narm_pool(hs, h_g, lengths, A1, A2, v):
    """narm_pool_fwd under autograd: c [B, H] whose backward hands back the kernel's gradients of hs, h_g, A1, A2 and v."""
    return _NarmPool.apply(hs, h_g, A1, A2, v.reshape(-1), _idx64(lengths, "lengths"))


def sgd_dense(tab, grad, lr, l2=0.0, stamp=None, step_id=0):
    abi.check(abi.lib().wr_sgd_dense(_p(_req(tab, torch.float32, "tab", 2)), tab.shape[0], tab.shape[1],
                                     _p(_req(grad, torch.float32, "grad", 2)), _p(stamp), step_id, lr, l2, _stream()),
              "wr_sgd_dense")


def adam_dense(tab, exp_avg, exp_avg_sq, grad, adam_step, lr, l2=0.0, beta1=0.9, beta2=0.999, eps=1e-8, stamp=None,
               step_id=0):
    for t, nm in ((tab, "tab"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq"), (grad, "grad")):
        _req(t, torch.float32, nm, 2)
    abi.check(abi.lib().wr_adam_dense(_p(tab), _p(exp_avg), _p(exp_avg_sq), tab.shape[0], tab.shape[1], _p(grad),
                                      _p(stamp), step_id, adam_step, lr, l2, beta1, beta2, eps, _stream()),
              "wr_adam_dense")


def _join_views(ts):
    """concatenation of 1-D tensors; free when they are adjacent views of the same storage"""
    if len(ts) == 1:
        return ts[0]
    a = ts[0]
    adjacent, end = a.is_contiguous(), a.storage_offset() + a.numel()
    for b in ts[1:]:
        adjacent = adjacent and b.is_contiguous() and b.dtype == a.dtype and \
            b.untyped_storage().data_ptr() == a.untyped_storage().data_ptr() and b.storage_offset() == end
        end += b.numel()
    if adjacent:
        return torch.as_strided(a, (end - a.storage_offset(),), (1,), a.storage_offset())
    return torch.cat(ts)


class PipelinedSgd:
    """Plain-SGD training over pre-ordered triplets with the plan build off the critical path.  The work is a list of
    segments (item table view + indices; one segment for a whole epoch on one GPU, one per part of the held block in the
    stratified multi-GPU schedule).  Batches are planned a chunk at a time on a side stream, one chunk ahead of the steps
    (a plan depends only on the indices, never on the tables) — across segment boundaries too — and a segment's steps are
    issued from native code (wr_bprmf_run_sgd).  A chunk is at least ``chunk`` batches and at least PLAN_TRIPLETS triplets
    (64 small batches do not amortise a plan's fixed host cost: scripts/exp/small_batch_pace.py, us/step with 64 batches per
    plan -> with 4 M triplets per plan: B = 2,048 11.1 -> 8.8, B = 16,384 17.8 -> 12.9; B = 65,536 is 64 batches either way).

    Nothing in the step stream waits on the host or allocates: plans are built into two pre-sized arenas (PlanArena) that
    alternate, and a plan's flags and hot-run counts come back through an asynchronous copy into pinned memory that is read
    when the plan's first step is queued — by then the build has long run, one chunk ahead (BatchPlan.finish)."""

    # Queue the build of the next plan behind the first N triplets' worth of steps of the current plan instead of behind all
    # of them (0 = off, the default).  It removes a bubble when queueing launches is slow — under rocprofv3 the host needs as
    # long to queue a 64-step chunk of the two-launch stream as the GPU to run it, and the build then starts when the steps end
    # (330 us of idle step stream per chunk in such a trace) — but on an unburdened host it costs: the driver's 20-step
    # command, same box, four runs each: off 30.3-32.8 us/step, 8 steps first 33.1-35.7, 16 steps first 31.5-37.3 (the build
    # then runs beside more of the steps, and the chunk's steps go out in two calls).
    PREFETCH_AFTER_TRIPLETS = 0
    PLAN_TRIPLETS = 1 << 22
    GROUP_MIN_ROWS_PER_TRIPLET = 12   # group plans (no per-batch sort): both tables hold at least this many rows per triplet of a
                                      # batch — with fewer, the lists of shared rows outgrow their capacity (uniform ids: a
                                      # share 1 - exp(-2 B / rows) of the item occurrences is shared: 15 % at 12 rows per triplet)
    GROUP_MIN_BATCH = 4096            # below this the step is launch-bound either way and the sorted plan's two tiny launches win

    CHAIN_MIN_BATCH = 8192        # below this the step is launch-bound: nothing to hide the item phase behind
    CHAIN_MIN_ITEMS_PER_TRIPLET = 6   # item rows per triplet of a batch: with fewer, too many runs are deferred (uniform ids:
                                      # 2 * (1 - exp(-x)(1 + x)), x = 2 B / rows, of the runs: 1/20 at 6 rows per triplet)

    def __init__(self, chunk=64, min_triplets=None, chain=True, inline_plan=False, group=True):
        """group (default): batches that qualify (int32 ids; 4,096 <= B <= 131,072; rows = whole 128-B lines; both tables large
        against the batch; no popularity-skewed ids) are NOT sorted at all: the plan only groups the rows that recur in a batch
        (GroupPlan, wr_group_plan_build: one launch per chunk, LDS bitmaps, ~0.1 B of plan per triplet) and the step is one
        launch (wr_bprmf_run_sgd_group).  A chunk whose lists overflow is re-planned with the sorted builder, and the stream
        stays with sorted plans from there on; so it does after a chunk that reports a long run.
        chain: steps of plans that qualify (no hot rows; B >= CHAIN_MIN_BATCH; rows = whole 128-B lines; item
        table large against the batch) go out as ONE launch per step — the item phase of step k-1 inside the launch of step
        k's user phase (wr_bprmf_run_sgd_chain; same tables bit for bit; MI355X, 1M x 1M x 64, B = 65,536, steps only:
        27.3 -> 24.7 us/step).
        inline_plan: build the plan of the NEXT chunk on the step stream itself, between the two halves of the current
        chunk's steps, instead of on a side stream beside them.  OFF by default — measured, not assumed: in a kernel trace of
        1M x 1M x 64, B = 65,536 the ~11 step kernels per chunk that overlap a plan kernel take 49 us instead of 24 (~280 us
        per chunk), which looks like a reason to serialise; but the plan of a chunk takes ~330 us when it runs alone (it is
        latency-bound: 32 K short workgroups), so in-stream costs MORE (29.9 against 29.4 us/step)."""
        import sys
        self.ops = sys.modules[__name__]
        self.chunk = int(chunk)
        self.chain = bool(chain)
        self.group = bool(group)
        self.inline_plan = inline_plan
        self.stats = {"plain_calls": 0, "chain_calls": 0, "group_calls": 0, "group_fallbacks": 0}
        self._garenas = {}
        if min_triplets is not None:
            self.PLAN_TRIPLETS = int(min_triplets)
        self.plan_stream = None
        self._arenas = {}

    def chunk_batches(self, batch_size):
        return max(self.chunk, self.PLAN_TRIPLETS // max(int(batch_size), 1))

    def _arena_pair(self, device, B, nb_total, overlap_items):
        """two arenas for plans of up to chunk_batches(B) batches of B triplets (never more than the work at hand), kept
        across epochs"""
        cap = min(self.chunk_batches(B), max(int(nb_total), 1)) * B
        key = (str(device), B, int(overlap_items))
        pair = self._arenas.get(key)
        if pair is None or pair[0].max_triplets < cap:
            pair = [self.ops.PlanArena(device, cap, B, overlap_items=overlap_items) for _ in range(2)]
            self._arenas[key] = pair
        return pair

    def _garena_pair(self, device, B, nb_total, n_users, n_items):
        cap = min(self.chunk_batches(B), max(int(nb_total), 1)) * B
        key = (str(device), B, int(n_users), int(n_items))
        pair = self._garenas.get(key)
        if pair is None or pair[0].max_triplets < cap:
            pair = [self.ops.GroupArena(device, cap, B, n_users, n_items) for _ in range(2)]
            self._garenas[key] = pair
        return pair

    def plan(self, U, segments, batch, first_chunk=None, lr=None, prep=None, runner=None):
        """segments: [(item rows view [rows, D], u, p, n)] — u rows of U, p and n rows of the view, in batch order.
        Only the last segment may end with a short batch.  first_chunk: batches in the first plan, or a list with the sizes
        of the first few plans (default: full chunks) — lets a caller that consumes the stream piecewise (bench.py: warm-up,
        then timed steps) put a plan boundary where its pieces meet.
        runner: callable(plan, first, count, losses) that issues `count` steps of `plan` from batch `first` — for updates
        other than plain SGD (the exact-lazy Adam / weight-decay steps, Adagrad, Adadelta: FusedOptimizer.run_batches); the
        plan pipeline (arenas, builds one chunk ahead on the side stream, asynchronous read-back) is the same."""
        if self.plan_stream is None:
            self.plan_stream = side_stream(U.device)
        B = int(batch)
        segs, first = [], 0
        for k, (rows, u, p, n) in enumerate(segments):
            nb = (u.numel() + B - 1) // B
            if u.numel() % B != 0 and any(s[1].numel() for s in segments[k + 1:]):
                raise ValueError("only the last segment may end with a short batch")
            segs.append({"tabs": self.ops.BprmfTables(U, rows) if nb else None, "nb": nb, "first": first})
            first += nb
        live = [s for s in segments if s[1].numel()]
        # one batch sequence across the segments: plan chunks are cut by size, not at segment ends (a plan holds indices
        # only; with short segments — 8-GPU strata of a few steps — that is 5x fewer plans and host syncs).  Segments that
        # are consecutive views of one array (the usual case: slices of an epoch's arrays) are joined without a copy.
        u_all, p_all, n_all = (_join_views([s[j] for s in live]) for j in (1, 2, 3))
        n_items = max([s[0].shape[0] for s in live] or [1])
        main = torch.cuda.current_stream(U.device)
        use_chain = self.chain and (runner is None or getattr(runner, "wants_chain_marks", False)) and \
            B >= self.CHAIN_MIN_BATCH and first >= 2 and \
            min([s[0].shape[0] for s in live] or [0]) >= self.CHAIN_MIN_ITEMS_PER_TRIPLET * B and \
            all(sg["tabs"].chain_supported() for sg in segs if sg["tabs"] is not None)
        min_rows = min([U.shape[0]] + [s[0].shape[0] for s in live])
        use_group = self.group and runner is None and len(live) == 1 and first >= 2 and \
            self.GROUP_MIN_BATCH <= B <= 131072 and u_all.dtype in (torch.int32, torch.int64) and \
            min_rows >= self.GROUP_MIN_ROWS_PER_TRIPLET * B and \
            all(sg["tabs"].group_supported() for sg in segs if sg["tabs"] is not None)
        garenas = self._garena_pair(U.device, B, first, U.shape[0], n_items) if use_group else None
        # the sorted plans' arenas are made on demand when a group-plan stream has to fall back (skewed ids)
        arenas = None if use_group else self._arena_pair(U.device, B, first, n_items if use_chain else 0)
        for a in (arenas or []) + (garenas or []):     # a previous handle may have left steps queued that read these arrays
            a.release_after(main)
        h = {"segs": segs, "B": B, "u": u_all, "p": p_all, "n": n_all, "nb": first, "n_users": U.shape[0], "n_items": n_items,
             "at": 0, "tag": 0, "next": None, "cur": None, "map": None, "arenas": arenas, "pos": 0,
             "group": use_group, "garenas": garenas, "device": U.device,
             # int64 columns (the reference's batch layout): the group plan and its step read int32 shadows, narrowed chunk by
             # chunk on the plan stream (12 B per triplet, once per epoch; the sorted plans read the int64 columns themselves)
             "ids32": [torch.empty(u_all.numel(), dtype=torch.int32, device=U.device) for _ in range(3)]
                      if use_group and u_all.dtype == torch.int64 else None,
             "chain": use_chain, "prep": prep, "runner": runner, "inline": bool(self.inline_plan),
             "lead": [int(c) for c in (first_chunk if isinstance(first_chunk, (list, tuple)) else [first_chunk or 0]) if c]}
        self.plan_stream.wait_stream(main)   # the index tensors are ready
        self._prefetch(h)
        return h

    def _build_stream(self, h):
        return torch.cuda.current_stream(h["u"].device) if h["inline"] else self.plan_stream

    def _prefetch(self, h):
        """enqueue the plan of the next chunk of batches on the side stream (no host wait, no allocation)"""
        if h["at"] >= h["nb"]:
            h["next"] = None
            return
        first, B = h["at"], h["B"]
        c = min(self.chunk_batches(B), h["nb"] - first)
        if h["lead"]:
            c = min(c, h["lead"].pop(0))
        h["at"] += c
        lo, hi = first * B, min(h["u"].numel(), (first + c) * B)
        with torch.cuda.stream(self._build_stream(h)):
            bmap = h["map"] if h["map"] else None
            if h["prep"] is not None:
                h["prep"].fill(lo, hi)       # this chunk's rows: shuffle + negatives, on the plan stream, before its plan
            if h["group"]:
                cols = (h["u"], h["p"], h["n"])
                if h["ids32"] is not None:
                    abi.check(abi.lib().wr_narrow_ids_i64(*[_p(c[lo:hi]) for c in cols], *[_p(c[lo:hi]) for c in h["ids32"]],
                                                          hi - lo, _stream()), "wr_narrow_ids_i64")
                    cols = h["ids32"]
                plan = self.ops.GroupPlan(cols[0][lo:hi], cols[1][lo:hi], cols[2][lo:hi], B, h["n_users"], h["n_items"],
                                          arena=h["garenas"][h["tag"]], defer=True)
                h["tag"] ^= 1
                h["next"] = (first, plan)
                return
            if h["arenas"] is None:          # first sorted plan of a stream that started with group plans
                h["arenas"] = self._arena_pair(h["device"], B, h["nb"], h["n_items"] if h["chain"] else 0)
            plan = self.ops.BatchPlan(h["u"][lo:hi], h["p"][lo:hi], h["n"][lo:hi], B, h["n_users"], h["n_items"],
                                      validate=False, ws_tag="rot%d" % h["tag"], bucket_map=bmap, arena=h["arenas"][h["tag"]],
                                      defer=True, overlap=h["chain"])
        h["tag"] ^= 1
        h["next"] = (first, plan)

    STICKY_MSG = "a wait inside a step launch expired (hand-off between the workgroups of one launch): the tables are not " \
                 "valid — do not save or evaluate them; restart the run"

    def _queue_sticky(self, h, tabs, main):
        """behind a chunk's last step: the launches' sticky timeout words -> pinned memory, asynchronously; read when the next
        chunk starts (or the run ends), i.e. before anything but ONE more chunk of steps can have used the tables"""
        words = tabs.sticky_words()
        if not words:
            return
        pin = h.get("sticky_pin")
        if pin is None or pin.numel() < 2 * len(words):
            pin = h["sticky_pin"] = torch.zeros(2 * max(len(words), 4), dtype=torch.int32, pin_memory=True)
        half = pin.numel() // 2
        off = half * (h.get("sticky_tag", 0) & 1)
        h["sticky_tag"] = h.get("sticky_tag", 0) + 1
        for j, wd in enumerate(words):
            pin[off + j:off + j + 1].copy_(wd, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(main)
        self._check_sticky(h)                       # at most one chunk's check is ever outstanding
        h["sticky_pending"] = (ev, pin[off:off + len(words)])

    def _check_sticky(self, h):
        pend = h.pop("sticky_pending", None)
        if pend is not None:
            pend[0].synchronize()
            if bool(pend[1].numpy().any()):
                raise abi.WhisprRecHipError(self.STICKY_MSG)

    def _take_next(self, h, pos, main):
        """the prefetched plan becomes the current one: its read-back is consumed here (flags, hot-run counts)"""
        self._check_sticky(h)
        if h["next"] is None:
            self._prefetch(h)
        cur = h["next"]
        assert cur is not None and cur[0] == pos, "steps must be run in order"
        plan = cur[1]
        plan.validate()                      # finish(): waits for the build's event only if the build has not run yet
        if isinstance(plan, GroupPlan):
            if plan.overflow or plan.long_run:
                # ids the group plan is not made for (tables small against the batch, popularity skew): sorted plans from
                # here on; after an overflow this chunk is re-planned too (its lists are incomplete)
                h["group"] = False
                self.stats["group_fallbacks"] += 1
                if h["next"] is not None and h["next"][0] != cur[0]:
                    raise AssertionError("plan pipeline out of step")
                if plan.overflow:
                    first, B = cur[0], h["B"]
                    lo, hi = first * B, first * B + plan.n_triplets
                    plan.arena.release_after(main)
                    if h["arenas"] is None:
                        h["arenas"] = self._arena_pair(h["device"], B, h["nb"], h["n_items"] if h["chain"] else 0)
                    with torch.cuda.stream(self._build_stream(h)):
                        plan = self.ops.BatchPlan(h["u"][lo:hi], h["p"][lo:hi], h["n"][lo:hi], B, h["n_users"], h["n_items"],
                                                  validate=False, ws_tag="rot%d" % h["tag"], arena=h["arenas"][h["tag"]],
                                                  defer=True, overlap=h["chain"])
                    h["tag"] ^= 1
                    plan.validate()
                    cur = (first, plan)
            main.wait_event(plan.ready)
            h["cur"], h["next"] = cur, None
            return cur
        main.wait_event(plan.ready)
        if plan.fast_overflowed:
            # skewed ids: equal-width buckets overflow chunk after chunk.  Balance the buckets by the rows' share of
            # the epoch (one pass over the id columns) and use them from the next chunk on; if even those overflow
            # (batches that are not random samples of the epoch), stay with the radix-sort builder.
            if plan._mapped():
                h["map"] = False
            elif h["map"] is None:
                with torch.cuda.stream(self._build_stream(h)):
                    # row shares from the whole epoch: with a pipelined preparation the batch-order columns are not
                    # complete yet, the source columns have the same rows in another order
                    src = (h["prep"].users, h["prep"].items) if h["prep"] is not None else (h["u"], h["p"])
                    h["map"] = self.ops.BucketMap(src[0], src[1], h["n_users"], h["n_items"], h["B"])
        if h["chain"] and plan.hot is not None:
            h["chain"] = False      # skewed ids stay skewed: the following plans skip the marks (hot batches take the two launches)
        if h["chain"] and plan.hot is None and plan.overlap is not None and not plan.overlap["fits"]:
            # ids that defer most runs (many shared item rows without any hot one): the marks are wasted plan work
            dcn = plan.overlap["def_count_np"]
            if int((dcn[1:] > plan.overlap["cap"]).sum()) * 2 > plan.n_batches - 1:
                h["chain"] = False
        h["cur"], h["next"] = cur, None
        return cur

    def _run_span(self, h, sg, pos, end, lr, losses, loss_off):
        """steps [pos, end) of the handle's batch sequence, all inside segment `sg`; losses[loss_off + k] for step pos + k"""
        main = torch.cuda.current_stream(sg["tabs"].U.device)
        while pos < end:
            cur = h["cur"]
            if cur is None or pos >= cur[0] + cur[1].n_batches:
                cur = self._take_next(h, pos, main)
            base, plan = cur
            c = min(end, base + plan.n_batches) - pos
            if h["inline"] and h["next"] is None and h["at"] < h["nb"]:
                # in-stream plan build: the next chunk's plan goes between the two halves of this chunk's steps
                mid = base + plan.n_batches // 2
                if pos >= mid:
                    self._prefetch(h)
                else:
                    c = min(c, mid - pos)
            elif self.PREFETCH_AFTER_TRIPLETS > 0 and h["next"] is None and h["at"] < h["nb"] and \
                    c > (self.PREFETCH_AFTER_TRIPLETS + h["B"] - 1) // h["B"]:
                c = (self.PREFETCH_AFTER_TRIPLETS + h["B"] - 1) // h["B"]      # see PREFETCH_AFTER_TRIPLETS
            if isinstance(plan, GroupPlan):
                sg["tabs"].run_sgd_group(plan, pos - base, c, lr, losses=losses[loss_off:loss_off + c])
                self.stats["group_calls"] += 1
            elif h["runner"] is not None:
                h["runner"](plan, pos - base, c, losses[loss_off:loss_off + c])
                self.stats["plain_calls"] += 1
            elif h["chain"] and plan.overlap is not None and c >= 2:
                sg["tabs"].run_sgd_chain(plan, pos - base, c, lr, losses=losses[loss_off:loss_off + c])
                self.stats["chain_calls"] += 1
            else:
                sg["tabs"].run_sgd(plan, pos - base, c, lr, losses=losses[loss_off:loss_off + c])
                self.stats["plain_calls"] += 1
            pos += c
            loss_off += c
            if pos >= base + plan.n_batches:
                plan.arena.release_after(main)                       # every step that reads the plan's arrays is queued
                self._queue_sticky(h, sg["tabs"], main)
            if h["next"] is None and not h["inline"]:
                self._prefetch(h)                                    # the next plan is built beside the queued steps
        h["pos"] = pos

    def run(self, handle, seg, lr, losses):
        """all steps of segment `seg` (segments must be run in order); losses: one slot per step"""
        sg = handle["segs"][seg]
        if sg["nb"] == 0:
            return
        self._run_span(handle, sg, sg["first"], sg["first"] + sg["nb"], lr, losses, 0)
        if seg == len(handle["segs"]) - 1:
            self._check_sticky(handle)      # the last chunk's word (waits for the stream: the caller is about to read the losses)

    def run_steps(self, handle, count, lr, losses):
        """the next `count` steps of a single-segment handle (a step stream consumed piecewise: warm-up, then the timed
        steps of bench.py — the plan pipeline runs on across the calls, as it does inside an epoch)"""
        assert len(handle["segs"]) == 1, "run_steps: single-segment handles"
        sg = handle["segs"][0]
        pos = handle["pos"]
        if pos + count > sg["nb"]:
            raise ValueError("run_steps: %d steps asked, %d left" % (count, sg["nb"] - pos))
        self._run_span(handle, sg, pos, pos + count, lr, losses, 0)


class LazyOptimizerState:
    """Exact lazy evaluation of torch.optim.Adam / SGD(weight_decay) on the two BPRMF tables (include/whisprrec_hip.h,
    "K5 (lazy, exact)"): per row the number of the last optimizer step applied to it; rows are replayed when a batch
    needs them and all together in ``flush()`` — call it before anything else reads the tables.  Bit-identical to the
    dense kernels (wr_adam_dense / wr_sgd_dense), without their table passes."""

    FOLD_MAX_GAP = 40      # fold the catch-up into the step kernels while a row misses about this many steps between two uses

    MAX_LAG = 64           # bounded lag (Adam): rows of a rotating window are replayed every step so that none misses more
    LAG_MIN_GAP = 64       # ... used when a row misses more than this many steps between two uses on average (rows / batch)

    def __init__(self, tabs, name, lr, l2, betas=(0.9, 0.999), eps=1e-8, fold=None, max_lag=None):
        """fold (Adam): the catch-up of a batch's rows happens inside the step kernels' row loads (wr_bprmf_step_adam_folded:
        6 instead of 12 row transfers per touched row) instead of in a pass of its own; same bits either way.  The folded
        replay is balanced over the four rows a wave holds (adam_replay_balanced: the wave transposes its data so that all
        64 lanes replay one row at a time — no team waits for the longest gap), but a row shared by several triplets is
        replayed by each of its readers, and with few waves on the GPU the replay is latency-bound, so it pays while replays are
        short: None (default) = fold when a row misses about FOLD_MAX_GAP steps or fewer between two batches that contain it
        (rows / batch size).  MI355X, 1M x 1M x 64, us/step separate -> folded: B = 65,536 (gap ~16) 155 -> 105; B = 32,768
        (~31) 105 -> 84; B = 16,384 (~61) 73 -> 91; B = 2,048 (~490) 55 -> 283 (scripts/ab_adam.py).
        max_lag (Adam, separate catch-up): None (default) = MAX_LAG when a row misses more than LAG_MIN_GAP steps between
        two uses on average, else unbounded; 0 = unbounded; n = before every step a rotating window of rows / n rows per
        table is brought up to date, so that no row ever misses more than n steps (wr_bprmf_run_adam_lazy_bounded).  Missed
        steps are geometrically distributed: at B = 2,048 on 1M-row tables the mean is ~490 and the longest among a batch's
        rows ~3,700 — one wave's serial chain that the whole launch waits for (steady state 206 us/step; the 44-56 us of
        short runs only hold until rows have been idle for long).  The window does the replays every row is owed anyway as
        uniform-length work over thousands of waves.  Same bits.  MI355X, 1M x 1M x 64, whole epochs in steady state
        (scripts/exp/adam_epoch.py), us/step at max_lag = unbounded / 1024 / 512 / 256 / 128 / 64 / 32 / 16: B = 2,048: 206 /
        151 / 96 / 76 / 66 / 61.6 / 62.4 / 78 (the window's row traffic grows as the lag shrinks); B = 8,192: - / 133 / 109 /
        - / 80 / 72.5 / 73.5 / 89; B = 16,384 (a row misses ~61 steps): 88 either way."""
        self.chain, self.chain_calls = True, 0     # folded Adam steps as one launch per step where the plan carries the marks
        if name not in ("SGD", "Adam"):
            raise ValueError(name)
        self.tabs, self.name, self.lr, self.l2, self.betas, self.eps = tabs, name, float(lr), float(l2), betas, float(eps)
        self.fold = fold if fold is None else bool(fold)
        self.max_lag = max_lag if max_lag is None else int(max_lag)
        self._sweep_pos = (ctypes.c_int64 * 2)(0, 0)
        dev = tabs.dev
        self.t = 0                                                       # optimizer steps taken
        self.flushed_at = 0
        self.last_u = torch.zeros(tabs.U.shape[0], dtype=torch.int32, device=dev)
        self.last_i = torch.zeros(tabs.I.shape[0], dtype=torch.int32, device=dev)
        if name == "Adam":
            z = torch.zeros_like
            self.m_u, self.v_u, self.m_i, self.v_i = z(tabs.U), z(tabs.U), z(tabs.I), z(tabs.I)
            self.consts = None
            self._grow_consts(4096)

    def _folds(self, plan):
        if self.fold is None:
            gap = max(self.tabs.U.shape[0], self.tabs.I.shape[0]) / float(max(plan.batch_size, 1))
            return gap <= self.FOLD_MAX_GAP
        return self.fold

    def _adam_state(self):
        return (_p(self.m_u), _p(self.v_u), _p(self.m_i), _p(self.v_i), _p(self.last_u), _p(self.last_i))

    def _grow_consts(self, n):
        host = torch.empty(2 * n, dtype=torch.float32)
        abi.check(abi.lib().wr_adam_consts(0, n, self.lr, self.betas[0], self.betas[1], host.data_ptr()), "wr_adam_consts")
        self.consts = host.to(self.tabs.dev)
        self.n_consts = n

    def _adam_rows(self, tab, m, v, last, keys_ptr, n_keys, grad):
        abi.check(abi.lib().wr_adam_rows_lazy(_p(tab), _p(m), _p(v), _p(last), tab.shape[0], tab.shape[1], keys_ptr, n_keys,
                                              _p(grad), self.t, _p(self.consts), self.n_consts, self.l2, self.betas[0],
                                              self.betas[1], self.eps, _stream()), "wr_adam_rows_lazy")

    def step(self, plan, k, loss_out=None):
        """optimizer step on batch k of the plan (gradient computation included); returns the loss tensor"""
        tabs = self.tabs
        if _auto_lag(self, plan) > 0 and not (self.name == "Adam" and self._folds(plan)):
            out = self.run(plan, k, 1, losses=None if loss_out is None else loss_out.reshape(1))   # keeps the window turning
            return out.reshape(()) if loss_out is None else loss_out
        self.t += 1
        batch = tabs._plan_ptrs(plan, k)
        tu, oi, B = batch[0], batch[3], batch[5]
        if self.name == "Adam":
            if self.t >= self.n_consts:
                self._grow_consts(2 * self.n_consts)
            hot = plan.hot_struct(k)
            folded = self._folds(plan) and hot is None
            if not folded:
                self._adam_rows(tabs.U, self.m_u, self.v_u, self.last_u, tu, B, None)       # the batch's rows up to t-1
                self._adam_rows(tabs.I, self.m_i, self.v_i, self.last_i, oi, 2 * B, None)
            # gradients + Adam on the rows the step kernels finish (no gradient table); folded: the catch-up rides in their loads
            loss_out = tabs._loss_buf(loss_out)
            ws = tabs._ws(plan.batch_size)
            head = (*tabs._table_head(), *self._adam_state(), *batch, self.t, self.lr)
            tail = (self.l2, self.betas[0], self.betas[1], self.eps, _p(loss_out))
            if folded:
                abi.check(abi.lib().wr_bprmf_step_adam_folded(*head, _p(self.consts), self.n_consts, *tail, _p(ws), ws.numel(),
                                                              _stream()), "wr_bprmf_step_adam_folded")
            else:
                abi.check(abi.lib().wr_bprmf_step_adam(*head, *tail, _addr(hot), _p(ws), ws.numel(), _stream()),
                          "wr_bprmf_step_adam")
            tabs.step_id += 1
            return loss_out
        L = abi.lib()
        for tab, last, keys, n in ((tabs.U, self.last_u, tu, B), (tabs.I, self.last_i, oi, 2 * B)):
            abi.check(L.wr_sgd_rows_lazy(_p(tab), _p(last), tab.shape[0], tab.shape[1], keys, n, self.t, self.lr, self.l2,
                                         _stream()), "wr_sgd_rows_lazy")
        return tabs.step_sgd(plan, k, self.lr, self.l2, loss_out=loss_out, decay_untouched=False)

    def run(self, plan, first, count, losses=None):
        """`count` consecutive optimizer steps on batches [first, first + count) of the plan, issued from native code
        (wr_bprmf_run_adam_lazy / wr_bprmf_run_sgd_lazy); same result as `count` calls of step()"""
        tabs, L = self.tabs, abi.lib()
        losses = tabs._loss_buf(losses, count)
        ws = tabs._ws(plan.batch_size)
        su, si = tabs._stamps()
        hot = plan.hot_struct()
        t0 = self.t + 1
        lag = _auto_lag(self, plan)
        if self.name == "Adam":
            while self.t + count >= self.n_consts:
                self._grow_consts(2 * self.n_consts)
            head = (*tabs._table_head(), *self._adam_state(), *tabs._plan_head(plan), first, count, t0, self.lr,
                    _p(self.consts), self.n_consts, self.l2, self.betas[0], self.betas[1], self.eps, _p(losses), _addr(hot))
            o = getattr(plan, "overlap", None)
            if self._folds(plan) and self.chain and o is not None and hot is None and count >= 2 and tabs.chain_supported():
                # one launch per step: the item phase of step k-1 inside the launch of step k's user phase
                ws2 = tabs.overlap_workspace(plan.batch_size)
                sync = tabs._chain_sync(count)
                abi.check(L.wr_bprmf_run_adam_folded_chain(*head[:-1], _p(o["tdef"]), _p(o["def_q"]),
                                                           o["def_count_host"].data_ptr(), o["cap"], o["cap"], _p(ws2),
                                                           ws2.numel(), _p(sync), sync.numel(), _stream()),
                          "wr_bprmf_run_adam_folded_chain")
                self.chain_calls += 1
            elif self._folds(plan):
                abi.check(L.wr_bprmf_run_adam_folded(*head, _p(ws), ws.numel(), _stream()), "wr_bprmf_run_adam_folded")
            elif lag > 0:
                abi.check(L.wr_bprmf_run_adam_lazy_bounded(*head, lag, _addr(self._sweep_pos), _p(ws), ws.numel(), _stream()),
                          "wr_bprmf_run_adam_lazy_bounded")
            else:
                abi.check(L.wr_bprmf_run_adam_lazy(*head, _p(ws), ws.numel(), _stream()), "wr_bprmf_run_adam_lazy")
        else:
            head = (*tabs._table_head(), _p(self.last_u), _p(self.last_i), _p(su), _p(si), tabs.step_id + 1,
                    *tabs._plan_head(plan), first, count, t0, self.lr, self.l2, _p(losses), _addr(hot))
            if lag > 0:
                abi.check(L.wr_bprmf_run_sgd_lazy_bounded(*head, lag, _addr(self._sweep_pos), _p(ws), ws.numel(), _stream()),
                          "wr_bprmf_run_sgd_lazy_bounded")
            else:
                abi.check(L.wr_bprmf_run_sgd_lazy(*head, _p(ws), ws.numel(), _stream()), "wr_bprmf_run_sgd_lazy")
        self.t += count
        tabs.step_id += count
        return losses

    def flush(self):
        """every row up to the current step: the tables are then what the dense optimizer would hold"""
        if self.flushed_at == self.t:
            return
        L, tabs = abi.lib(), self.tabs
        if self.name == "Adam":
            for tab, m, v, last in ((tabs.U, self.m_u, self.v_u, self.last_u), (tabs.I, self.m_i, self.v_i, self.last_i)):
                abi.check(L.wr_adam_catchup_all(_p(tab), _p(m), _p(v), _p(last), *tab.shape, self.t, _p(self.consts),
                                                self.n_consts, self.l2, self.betas[0], self.betas[1], self.eps, _stream()),
                          "wr_adam_catchup_all")
        else:
            for tab, last in ((tabs.U, self.last_u), (tabs.I, self.last_i)):
                abi.check(L.wr_sgd_catchup_all(_p(tab), _p(last), *tab.shape, self.t, self.lr, self.l2, _stream()),
                          "wr_sgd_catchup_all")
        self.flushed_at = self.t


class StatefulSparseState:
    """torch.optim.Adagrad / Adadelta (weight_decay = 0) fused into the step kernels (wr_bprmf_run_stateful): with a zero
    gradient neither moves a weight, so only the rows of a batch are touched and the tables are always current (nothing to
    flush).  Adagrad's state (state_sum) is exactly sparse; Adadelta's two state rows decay by rho at every step — the
    missed decays of a row are replayed when it is next updated (``last`` = step of its last update)."""

    KIND = {"Adagrad": 1, "Adadelta": 2}

    MAX_LAG, LAG_MIN_GAP = 64, 64       # Adadelta: bounded lag as in LazyOptimizerState

    def __init__(self, tabs, name, lr, rho=0.9, eps=None, max_lag=None):
        """max_lag (Adadelta): a rotating window of rows / max_lag rows per table takes its missed decays before every step
        (wr_bprmf_run_stateful_bounded) — None = MAX_LAG when a row misses more than LAG_MIN_GAP steps on average, 0 = never."""
        if name not in self.KIND:
            raise ValueError(name)
        self.max_lag = max_lag if max_lag is None else int(max_lag)
        self._sweep_pos = (ctypes.c_int64 * 2)(0, 0)
        self.tabs, self.name, self.lr, self.rho = tabs, name, float(lr), float(rho)
        self.eps = float(eps) if eps is not None else (1e-10 if name == "Adagrad" else 1e-6)   # torch.optim defaults
        z = torch.zeros_like
        self.s1_u, self.s1_i = z(tabs.U), z(tabs.I)
        self.s2_u = self.s2_i = self.last_u = self.last_i = None
        if name == "Adadelta":
            self.s2_u, self.s2_i = z(tabs.U), z(tabs.I)
            self.last_u = torch.zeros(tabs.U.shape[0], dtype=torch.int32, device=tabs.dev)
            self.last_i = torch.zeros(tabs.I.shape[0], dtype=torch.int32, device=tabs.dev)
        self.t = 0

    def run(self, plan, first, count, losses=None):
        tabs = self.tabs
        losses = tabs._loss_buf(losses, count)
        ws = tabs._ws(plan.batch_size)
        hot = plan.hot_struct()
        head = (self.KIND[self.name], *tabs._table_head(), _p(self.s1_u), _p(self.s2_u), _p(self.s1_i), _p(self.s2_i),
                _p(self.last_u), _p(self.last_i), *tabs._plan_head(plan), first, count, self.t + 1, self.lr, self.rho, self.eps,
                _p(losses), _addr(hot))
        lag = _auto_lag(self, plan)
        if self.name == "Adadelta" and lag > 0:
            abi.check(abi.lib().wr_bprmf_run_stateful_bounded(*head, lag, _addr(self._sweep_pos), _p(ws), ws.numel(), _stream()),
                      "wr_bprmf_run_stateful_bounded")
        else:
            abi.check(abi.lib().wr_bprmf_run_stateful(*head, _p(ws), ws.numel(), _stream()), "wr_bprmf_run_stateful")
        self.t += count
        tabs.step_id += count
        return losses

    def step(self, plan, k, loss_out=None):
        out = self.run(plan, k, 1, losses=None if loss_out is None else loss_out.reshape(1))
        return out.reshape(()) if loss_out is None else loss_out

    def flush(self):
        """nothing to do: the weights never lag (kept so that callers treat every optimizer state alike)"""


def adam_consts(n, lr, beta1=0.9, beta2=0.999, device=None):
    """device table of the per-step Adam constants for steps 0..n-1 (wr_adam_consts: the host expressions of wr_adam_dense)"""
    host = torch.empty(2 * n, dtype=torch.float32)
    abi.check(abi.lib().wr_adam_consts(0, n, lr, beta1, beta2, host.data_ptr()), "wr_adam_consts")
    return host.to(device) if device is not None else host


def adam_dense_dev(tab, exp_avg, exp_avg_sq, grad, consts, step_dev, l2=0.0, beta1=0.9, beta2=0.999, eps=1e-8):
    """wr_adam_dense with the step number read from device memory (graph-replayable)"""
    for t, nm in ((tab, "tab"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq"), (grad, "grad")):
        _req(t, torch.float32, nm, 2)
    abi.check(abi.lib().wr_adam_dense_dev(_p(tab), _p(exp_avg), _p(exp_avg_sq), tab.shape[0], tab.shape[1], _p(grad),
                                          _p(consts), consts.numel() // 2, _p(step_dev), l2, beta1, beta2, eps, _stream()),
              "wr_adam_dense_dev")


def adam_dense_dev_pair(a, b, consts, step_dev, l2=0.0, beta1=0.9, beta2=0.999, eps=1e-8):
    """adam_dense_dev for two tables of the same width in one launch; a, b: (tab, exp_avg, exp_avg_sq, grad)"""
    for grp in (a, b):
        for t, nm in zip(grp, ("tab", "exp_avg", "exp_avg_sq", "grad")):
            _req(t, torch.float32, nm, 2)
    if a[0].shape[1] != b[0].shape[1]:
        raise ValueError("adam_dense_dev_pair: tables of different width")
    abi.check(abi.lib().wr_adam_dense_dev_pair(_p(a[0]), _p(a[1]), _p(a[2]), a[0].shape[0], _p(a[3]), _p(b[0]), _p(b[1]), _p(b[2]),
                                               b[0].shape[0], _p(b[3]), a[0].shape[1], _p(consts), consts.numel() // 2,
                                               _p(step_dev), l2, beta1, beta2, eps, _stream()), "wr_adam_dense_dev_pair")


def counter_add(counter, delta=1):
    abi.check(abi.lib().wr_counter_add(_p(_req(counter, torch.int32, "counter", 1)), int(delta), _stream()), "wr_counter_add")


# ----------------------------------------------------------------------------------------------- rows
def gather_rows(tab, idx):
    """nn.Embedding forward: out[..., :] = tab[idx[...], :]."""
    _req(tab, torch.float32, "tab", 2)
    flat = _idx64(idx.reshape(-1), "idx")
    out = torch.empty((flat.numel(), tab.shape[1]), dtype=torch.float32, device=tab.device)
    abi.check(abi.lib().wr_gather_rows(_p(tab), tab.shape[0], tab.shape[1], _p(flat), flat.numel(), _p(out), _stream()),
              "wr_gather_rows")
    return out.reshape(tuple(idx.shape) + (tab.shape[1],))


def scatter_add_rows(grad, idx, src, padding_idx=-1, alpha=1.0):
    """embedding_dense_backward: grad[idx[k], :] += alpha * src[k, :] for idx[k] != padding_idx (in place)."""
    _req(grad, torch.float32, "grad", 2)
    flat = _idx64(idx.reshape(-1), "idx")
    src2 = _req(src.reshape(flat.numel(), grad.shape[1]).contiguous(), torch.float32, "src", 2)
    if flat.numel() == 0:
        return grad
    L = abi.lib()
    nbytes = abi.check_size(L.wr_scatter_add_workspace_bytes(flat.numel(), grad.shape[0]),
                            "wr_scatter_add_workspace_bytes")
    ws = workspace(grad.device, "scatter").get(nbytes)
    abi.check(L.wr_scatter_add_rows(_p(grad), grad.shape[0], grad.shape[1], _p(flat), _p(src2), flat.numel(),
                                    padding_idx, alpha, _p(ws), ws.numel(), _stream()), "wr_scatter_add_rows")
    return grad


# ------------------------------------------------------------------------------------------ row-lazy optimizers (K22, K24)
ROW_ERR_ID, ROW_ERR_PERM = 1, 2          # bits of the kernels' device error word


def _raise_row_errors(err, what):
    """one read of a device error word of the K22 kernels; clears it and raises IndexError if a bit is set"""
    word = int(err.item())
    if word:
        err.zero_()
        raise IndexError("%s: %s" % (what, " and ".join(
            t for bit, t in ((ROW_ERR_ID, "a row id outside the table"), (ROW_ERR_PERM, "a position outside the step's rows"))
            if word & bit)))


def rows_sparse_order(idx, n_rows, err_word=None):
    """(row, position) order of a step's positions: -> (sorted_rows int32 [n], perm int64 [n]).  The keys come from
    wr_rows_sparse_keys (ids outside the table: key n_rows, bit 1 of the error word); the ordering itself is a stable
    torch.sort of the 32-bit keys ("Row-lazy item table": the library's sorting stages are private to
    wr_scatter_add_rows and produce its tile / plan layouts, not one sorted list)."""
    flat = _idx64(idx.reshape(-1), "idx")
    keys = torch.empty(flat.numel(), dtype=torch.int32, device=flat.device)
    abi.check(abi.lib().wr_rows_sparse_keys(_p(flat), flat.numel(), int(n_rows), _p(keys), _p(err_word), _stream()),
              "wr_rows_sparse_keys")
    if flat.numel() == 0:
        return keys, torch.empty(0, dtype=torch.int64, device=flat.device)
    return torch.sort(keys, stable=True)


class RowLazyTable:
    """torch.optim.Adam / SGD(weight_decay) on a table whose gradient arrives as (index, gradient row) pairs (wr_rowopt.hip;
    include/whisprrec_hip.h, K22 and K24).  Every row carries the number of the last optimizer step applied to it; ``gather``
    returns rows as of the current step without writing anything, ``step`` moves the rows of the step only, ``flush`` brings
    all rows up to date — call it before anything else reads ``weight``.  Two faces:
      ONE table (the item table of the sequential models): after a flush, weight and moments hold the bits of "zero table,
        scatter_add_rows, adam_dense / sgd_dense" repeated step by step.  Under SGD without decay an untouched row never moves:
        no state.
      a PAIR (``target`` given: BUIR's online and target tables): the target follows the online table by ``target =
        target*momentum + weight*(1 - momentum)`` after every optimizer step; one step number per row counts optimizer steps and
        target updates together, ``gather`` returns both rows, ``step`` ends with the target update of its rows, and after a
        flush the target too holds the bits of the dense loop with ``ema_update_``.  Always stateful: the target of an
        untouched row moves even under SGD without decay."""

    MAX_LAG, LAG_MIN_GAP = LazyOptimizerState.MAX_LAG, LazyOptimizerState.LAG_MIN_GAP
    # the entry of an operation by (Adam, pair)
    ENTRIES = {"gather": {(True, False): "wr_gather_rows_lazy", (False, False): "wr_gather_rows_lazy_sgd",
                          (True, True): "wr_gather_rows_ema", (False, True): "wr_gather_rows_ema_sgd"},
               "step": {(True, False): "wr_adam_rows_sparse", (False, False): "wr_sgd_rows_sparse",
                        (True, True): "wr_adam_rows_sparse_ema", (False, True): "wr_sgd_rows_sparse_ema"},
               "catchup": {(True, False): "wr_adam_catchup_all", (False, False): "wr_sgd_catchup_all",
                           (True, True): "wr_adam_catchup_ema", (False, True): "wr_sgd_catchup_ema"}}

    def __init__(self, weight, name, lr, l2, betas=(0.9, 0.999), eps=1e-8, max_lag=None, padding_idx=-1, target=None,
                 momentum=None):
        """max_lag as for LazyOptimizerState: None = MAX_LAG when a row misses more than LAG_MIN_GAP steps between two uses on
        average (rows / positions of the step), 0 = unbounded, n = before every step a rotating window of rows / n rows is
        brought up to date, so that no row ever lags more than n.  momentum (with target) as ema_update_ takes it: rounded to
        fp32, 1 - momentum formed in double.  A pair has no padding row."""
        if name not in ("SGD", "Adam"):
            raise ValueError(name)
        _req(weight, torch.float32, "weight", 2)
        self.tgt = self.mom = self.one_minus_mom = None
        if target is not None:
            _req(target, torch.float32, "target", 2)
            if target.shape != weight.shape:
                raise ValueError("target and weight must have one shape (got %s and %s)" % (tuple(target.shape), tuple(weight.shape)))
            if momentum is None or int(padding_idx) != -1:
                raise ValueError("a pair of tables needs a momentum and has no padding row")
            self.tgt, self.mom, self.one_minus_mom = target, float(momentum), float(1. - float(momentum))
        elif momentum is not None:
            raise ValueError("momentum without a target")
        self.w, self.name, self.lr, self.l2 = weight, name, float(lr), float(l2)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.max_lag = max_lag if max_lag is None else int(max_lag)
        self.padding_idx = int(padding_idx)
        self.t = 0                               # optimizer steps (and target updates) taken
        self.flushed_at = 0
        self._sweep = 0                          # first row of the next window
        dev = weight.device
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)
        self.stateful = name == "Adam" or self.l2 != 0.0 or target is not None
        self.m = self.v = self.last = self.consts = None
        if self.stateful:
            self.last = torch.zeros(weight.shape[0], dtype=torch.int32, device=dev)
        if name == "Adam":
            self.m, self.v = torch.zeros_like(weight), torch.zeros_like(weight)
            self._grow_consts(4096)

    def _grow_consts(self, n):
        host = torch.empty(2 * n, dtype=torch.float32)
        abi.check(abi.lib().wr_adam_consts(0, n, self.lr, self.betas[0], self.betas[1], host.data_ptr()), "wr_adam_consts")
        self.consts = host.to(self.w.device)
        self.n_consts = n

    def _call(self, op, lo, n_rows, mid, tail=()):
        """one entry of wr_rowopt.hip / wr_lazy.hip, by this table's optimizer and face: (the tables from row lo on, n_rows, D,
        *mid, the optimizer's constants, *tail, stream)"""
        adam, pair = self.name == "Adam", self.tgt is not None
        entry = self.ENTRIES[op][adam, pair]
        tabs = [self.w] + ([self.tgt] if pair else []) + ([self.m, self.v] if adam else []) + [self.last]
        opt = (_p(self.consts), self.n_consts, self.l2, *self.betas, self.eps) if adam else (self.lr, self.l2)
        if pair:
            opt += (self.mom, self.one_minus_mom)
        abi.check(getattr(abi.lib(), entry)(*(_p(t[lo:] if lo else t) for t in tabs), n_rows, self.w.shape[1], *mid, *opt, *tail,
                                            _stream()), entry)

    def check(self):
        """one read of the device error word that unchecked gathers and steps leave their findings in"""
        _raise_row_errors(self.err, type(self).__name__)

    def gather(self, idx, check=True):
        """rows idx[...] as of step t; a pair: -> (online rows, target rows).  check: ids outside the table raise IndexError here
        (one device read); else they come back as zero rows and the finding waits in the error word for check() / flush()."""
        if not self.stateful:
            if check:
                flat = idx.reshape(-1)
                if flat.numel() and (int(flat.min()) < 0 or int(flat.max()) >= self.w.shape[0]):
                    raise IndexError("RowLazyTable: a row id outside the table")
            return gather_rows(self.w, idx)
        flat = _idx64(idx.reshape(-1), "idx")
        n, (n_rows, D) = flat.numel(), self.w.shape
        outs = [torch.empty((n, D), dtype=torch.float32, device=self.w.device) for _ in range(1 if self.tgt is None else 2)]
        self._call("gather", 0, n_rows, (_p(flat), n, self.t), (*map(_p, outs), _p(self.err)))
        if check:
            self.check()
        outs = [o.reshape(tuple(idx.shape) + (D,)) for o in outs]
        return outs[0] if self.tgt is None else tuple(outs)

    def _catchup(self, lo, count, upto):
        """rows [lo, lo + count) up to step `upto` (zero gradients; a pair: every step followed by its target update)"""
        self._call("catchup", lo, count, (upto,))

    def _lag(self, n_positions):
        if self.max_lag is None:
            return self.MAX_LAG if self.w.shape[0] / float(max(n_positions, 1)) > self.LAG_MIN_GAP else 0
        return self.max_lag

    def _turn_window(self, lag, upto):
        """the rotating window of ceil(rows / lag) rows -> step `upto`, in up to two pieces across the wrap-around"""
        n_rows = self.w.shape[0]
        left, lo = min((n_rows + lag - 1) // lag, n_rows), self._sweep % n_rows
        while left > 0:
            c = min(left, n_rows - lo)
            self._catchup(lo, c, upto)
            lo, left = (lo + c) % n_rows, left - c
        self._sweep = lo

    def _order(self, idx_list, grad_list, check):
        """the step's positions in (row, position) order -> (n, sorted rows, perm, gradient rows), lists concatenated"""
        who = type(self).__name__
        if len(idx_list) != len(grad_list):
            raise ValueError("%s.step: as many index tensors as gradient tensors" % who)
        n_rows, D = self.w.shape
        idx = [_idx64(i.reshape(-1), "idx") for i in idx_list]
        grads = [g.reshape(-1, D) for g in grad_list]
        for i, g in zip(idx, grads):
            if g.shape[0] != i.numel():
                raise ValueError("%s.step: %d gradient rows for %d indices" % (who, g.shape[0], i.numel()))
        n = sum(i.numel() for i in idx)
        if not n:
            return 0, None, None, None
        cat = torch.cat(idx) if len(idx) > 1 else idx[0]
        rows, perm = rows_sparse_order(cat, n_rows, err_word=self.err)
        if check:
            self.check()
        return n, rows, perm, _req((torch.cat(grads) if len(grads) > 1 else grads[0]).contiguous(), torch.float32, "grad", 2)

    def _window(self, n, t):
        """before step t with n positions: the constants of step t, and the rotating window up to step t - 1"""
        if not self.stateful:
            return
        if self.name == "Adam" and t >= self.n_consts:
            self._grow_consts(2 * self.n_consts)
        lag = self._lag(n)
        if lag > 0 and t > 1:
            self._turn_window(lag, t - 1)

    def _apply(self, n, rows, perm, src, t):
        """step t (a pair: and its target update) on the rows of the step"""
        if n:
            pad = () if self.tgt is not None else (self.padding_idx,)
            self._call("step", 0, self.w.shape[0], (_p(rows), _p(perm), n, _p(src), *pad, t), (_p(self.err),))

    def step(self, idx_list, grad_list, check=True):
        """optimizer step t + 1 (a pair: and its target update) with the gradient rows grad_list[i][k, :] of the rows
        idx_list[i][k]: the lists are concatenated in list order (the order of the forward lookups), brought into (row, position)
        order, the window is turned and the step's rows are moved.  A step without positions still counts.  check: an id outside
        the table raises IndexError before anything is written."""
        n, rows, perm, src = self._order(idx_list, grad_list, check)
        t = self.t + 1
        self._window(n, t)
        self._apply(n, rows, perm, src, t)
        self.t = t

    def flush(self):
        """every row up to step t: weight, the moments and a pair's target are then what the dense optimizer (and ema_update_)
        hold.  A no-op when nothing happened since the last flush.  Also where the findings of unchecked calls are raised."""
        if self.flushed_at != self.t:
            if self.stateful:
                self._catchup(0, self.w.shape[0], self.t)
            self.flushed_at = self.t
            self.check()

    def behind(self):
        """steps the most outdated row lags behind (one device read)"""
        return self.t - int(self.last.min()) if self.stateful else 0


class RowLazyEmaTable(RowLazyTable):
    """RowLazyTable's pair face under the name and with the constructor BUIR's optimizer uses"""

    def __init__(self, weight, target, name, lr, l2, momentum, betas=(0.9, 0.999), eps=1e-8, max_lag=None):
        super().__init__(weight, name, lr, l2, betas, eps, max_lag, target=target, momentum=momentum)


class ScatterPlan:
    """Row plan of several scatter-adds whose indices are known ahead (wr_scatter.hip): idx [n_segments, seg_stride] int64
    (segment s uses its first seg_len[s] positions; seg_len int32 on the device, or None = all).  ``apply(table, s, n, src,
    alpha)`` is then ONE launch.  ``slow`` (read with the caller's own read-back of ``meta``): some range of rows was not
    listed and is summed by brute force — exact, slow; callers with such ids stay with scatter_add_rows' sorted path."""

    def __init__(self, idx, n_rows, seg_len=None, padding_idx=-1):
        L = abi.lib()
        _req(idx, torch.int64, "idx", 2)
        self.idx = idx.contiguous()
        self.n_segments, self.stride = self.idx.shape
        self.n_rows, self.padding_idx = int(n_rows), int(padding_idx)
        words = int(L.wr_scatter_plan_words(self.n_segments, self.stride, self.n_rows))
        if words <= 0:
            raise ValueError("row plan not applicable: segments of %d positions" % self.stride)
        if seg_len is not None:
            seg_len = _req(seg_len.contiguous(), torch.int32, "seg_len", 1)
            assert seg_len.numel() == self.n_segments
        self.buf = torch.empty(words, dtype=torch.int32, device=idx.device)
        abi.check(L.wr_scatter_plan_build(_p(self.idx), self.n_segments, self.stride, _p(seg_len), self.n_rows,
                                          self.padding_idx, _p(self.buf), words, _stream()), "wr_scatter_plan_build")
        self.meta = self.buf[:4]

    @property
    def slow(self):
        return bool(int(self.meta[1].item()) != 0)

    def apply(self, table, segment, n, src, alpha=1.0):
        _req(table, torch.float32, "table", 2)
        _req(src, torch.float32, "src", 2)
        assert table.shape[0] == self.n_rows and src.shape[0] >= n and src.shape[1] == table.shape[1] and src.is_contiguous()
        abi.check(abi.lib().wr_scatter_add_planned(_p(table), self.n_rows, table.shape[1], _p(self.idx), self.n_segments,
                                                   self.stride, int(segment), int(n), self.padding_idx, _p(src), float(alpha),
                                                   _p(self.buf), self.buf.numel(), _stream()), "wr_scatter_add_planned")
        return table


# ----------------------------------------------------------------------------------------------- LightGCN pieces
def spmm_csr(row_ptr, col, val, X, Y=None, acc=None):
    _req(row_ptr, torch.int64, "row_ptr", 1)
    _req(col, torch.int32, "col", 1)
    _req(val, torch.float32, "val", 1)
    _req(X, torch.float32, "X", 2)
    if Y is None:
        Y = torch.empty_like(X)
    abi.check(abi.lib().wr_spmm_csr(X.shape[0], _p(row_ptr), _p(col), _p(val), _p(X), X.shape[1], _p(Y), _p(acc),
                                    _stream()), "wr_spmm_csr")
    return Y


SPMM_CHUNK_NNZ = 96              # non-zeros per chunk of the load-balanced CSR product
SPMM_ONE_LEVEL_MAX_CHUNKS = 48   # one combine level while no row has more chunks than this
SPMM_FUSED_COMBINE = False       # True: one-level products in ONE launch (wr_spmm_csr_chunked_fused: the last chunk of a cut
                                 # row to finish combines; D % 32 == 0).  Same bits; measured, not adopted: every chunk of a cut
                                 # row waits for its write-through store and for a returning atomic (~3 us of a wave's ~8 us
                                 # life).  ml-1m-shaped graphs, us per product fused / two launches: 1.41 M non-zeros, chunks of
                                 # 64 / 96 / 128 / 192: 63.4 / 38.7, 48.7 / 34.4, 43.2 / 37.7, 42.5 / 48.1; 0.71 M non-zeros
                                 # (C3 epoch): 35.0 against 35.8 ms per epoch (scripts/exp/spmm_fused_ab.py)


def spmm_chunks(row_ptr, max_nnz=SPMM_CHUNK_NNZ):
    """Cut CSR rows into chunks of at most `max_nnz` non-zeros (host, once per graph).  Returns (chunk_ptr int64
    [n_chunks+1], chunk_row int32 [n_chunks]) as CPU tensors; every row gets at least one chunk.  chunk_row carries the
    number of combine levels spmm_csr_chunked should use (``_wr_levels``: 1 while no row has more than
    SPMM_ONE_LEVEL_MAX_CHUNKS chunks).  MI355X, ml-1m-shaped graph (1.41 M non-zeros, hub rows of 3.4 K), us per product
    (scripts/ab_spmm.py), two levels / one level: 32 per chunk 39.3 / 41.2; 64: 37.6 / 34.8; 96: 34.9 / 31.5; 128: 35.8 /
    32.4; 192: 44 / 41; 256: 48 / 45."""
    import numpy as np
    rp = row_ptr.cpu().numpy() if isinstance(row_ptr, torch.Tensor) else np.asarray(row_ptr)
    deg = np.diff(rp)
    per = np.maximum(1, (deg + max_nnz - 1) // max_nnz)
    chunk_row = np.repeat(np.arange(len(deg), dtype=np.int32), per)
    first = np.cumsum(per) - per                       # index of each row's first chunk
    within = np.arange(chunk_row.size) - np.repeat(first, per)
    start = rp[:-1][chunk_row] + within * max_nnz
    chunk_ptr = np.concatenate([start, rp[-1:]]).astype(np.int64)
    crow = torch.from_numpy(chunk_row)
    crow._wr_levels = 1 if int(per.max(initial=1)) <= SPMM_ONE_LEVEL_MAX_CHUNKS else 2
    return torch.from_numpy(chunk_ptr), crow


def spmm_levels_of(chunk_row):
    """combine levels for a chunk_row tensor (the attribute set by spmm_chunks does not survive .to(device): recomputed once
    per tensor from the longest run of equal rows)"""
    lv = getattr(chunk_row, "_wr_levels", None)
    if lv is None:
        cr = chunk_row
        if cr.numel() <= 1:
            lv = 1
        else:
            change = torch.nonzero(cr[1:] != cr[:-1]).flatten() + 1
            edges = torch.cat([change.new_zeros(1), change, change.new_full((1,), cr.numel())])
            lv = 1 if int((edges[1:] - edges[:-1]).max()) <= SPMM_ONE_LEVEL_MAX_CHUNKS else 2
        chunk_row._wr_levels = lv
    return lv


def spmm_csr_chunked(chunk_ptr, chunk_row, col, val, X, Y=None, acc=None, partials=None, levels=None, acc_from_x=False,
                     acc_scale=1.0):
    """Y = A X (load-balanced CSR product); acc: running layer sum, acc = (acc + Y) * acc_scale, or (X + Y) * acc_scale with
    acc_from_x (first layer of a propagation: acc need not be initialised)."""
    _req(chunk_ptr, torch.int64, "chunk_ptr", 1)
    _req(chunk_row, torch.int32, "chunk_row", 1)
    _req(col, torch.int32, "col", 1)
    _req(val, torch.float32, "val", 1)
    _req(X, torch.float32, "X", 2)
    if Y is None:
        Y = torch.empty_like(X)
    if partials is None:
        partials = torch.empty((chunk_row.numel(), X.shape[1]), dtype=torch.float32, device=X.device)
    lv = spmm_levels_of(chunk_row) if levels is None else int(levels)
    if SPMM_FUSED_COMBINE and lv == 1 and X.shape[1] % 32 == 0 and partials.data_ptr() % 128 == 0:
        # one launch: the last chunk of a cut row to finish adds the row's partials (wr_spmm_csr_chunked_fused)
        st = getattr(chunk_row, "_wr_fuse", None)
        if st is None:
            per = torch.bincount(chunk_row.long(), minlength=X.shape[0])
            span = torch.stack([torch.cumsum(per, 0) - per, per], dim=1).to(torch.int32).reshape(-1).contiguous()
            st = chunk_row._wr_fuse = (span, torch.zeros(X.shape[0], dtype=torch.int32, device=X.device))
        abi.check(abi.lib().wr_spmm_csr_chunked_fused(X.shape[0], chunk_row.numel(), _p(chunk_ptr), _p(chunk_row), _p(st[0]),
                                                      _p(col), _p(val), _p(X), X.shape[1], _p(Y), _p(acc), _p(partials), None,
                                                      1 if acc_from_x else 0, float(acc_scale), _p(st[1]), _stream()),
                  "wr_spmm_csr_chunked_fused")
        return Y
    abi.check(abi.lib().wr_spmm_csr_chunked_levels(X.shape[0], chunk_row.numel(), _p(chunk_ptr), _p(chunk_row), _p(col),
                                                   _p(val), _p(X), X.shape[1], _p(Y), _p(acc), _p(partials), None,
                                                   lv, 1 if acc_from_x else 0, float(acc_scale), _stream()),
              "wr_spmm_csr_chunked_levels")
    return Y


# ----------------------------------------------------------------------------------------------- SGL views on the device
SGL_VIEW_BASE_CHUNK = 64         # base edges per wave of the view builder (wr_views.hip: one ballot per chunk)
SGL_VIEW_KINDS = {"ED": 0, "ND": 1}


def _chunks_count(row_ptr):
    """first half of spmm_chunks on the device -> (chunk_first int64 [n_rows + 1], max_per int32 [1]); nothing is read back"""
    _req(row_ptr, torch.int64, "row_ptr", 1)
    n_rows = row_ptr.numel() - 1
    dev = row_ptr.device
    per = torch.empty(n_rows, dtype=torch.int64, device=dev)
    max_per = torch.zeros(1, dtype=torch.int32, device=dev)
    abi.check(abi.lib().wr_spmm_chunks_count(_p(row_ptr), n_rows, SPMM_CHUNK_NNZ, _p(per), _p(max_per), _stream()),
              "wr_spmm_chunks_count")
    chunk_first = torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
    torch.cumsum(per, 0, out=chunk_first[1:])
    return chunk_first, max_per


def _chunks_fill(row_ptr, chunk_first, n_chunks, max_per):
    """second half: the tables for the sizes read back -> (chunk_ptr, chunk_row) with ``_wr_levels`` set"""
    dev = row_ptr.device
    chunk_ptr = torch.empty(n_chunks + 1, dtype=torch.int64, device=dev)
    chunk_row = torch.empty(n_chunks, dtype=torch.int32, device=dev)
    abi.check(abi.lib().wr_spmm_chunks_fill(_p(row_ptr), row_ptr.numel() - 1, SPMM_CHUNK_NNZ, _p(chunk_first), n_chunks,
                                            _p(chunk_ptr), _p(chunk_row), _stream()), "wr_spmm_chunks_fill")
    chunk_row._wr_levels = 1 if int(max_per) <= SPMM_ONE_LEVEL_MAX_CHUNKS else 2
    return chunk_ptr, chunk_row


def spmm_chunks_device(row_ptr):
    """spmm_chunks for a row_ptr that lives on the device (wr_spmm_chunks_count / _fill): the same (chunk_ptr, chunk_row), as
    device tensors, chunk_row carrying ``_wr_levels``.  One read-back (number of chunks, longest row)."""
    chunk_first, max_per = _chunks_count(row_ptr)
    n_chunks, mp = torch.cat([chunk_first[-1:], max_per.to(torch.int64)]).tolist()
    return _chunks_fill(row_ptr, chunk_first, n_chunks, mp)


class SglViewsBase:
    """The device-resident base of SGL's views (sgl_views_base): uploaded once per model"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def sgl_views_base(rows, cols, n_nodes, device):
    """Upload the base of the device view builder: the directed edge list (rows, cols) of the symmetric adjacency over n_nodes
    nodes, sorted by (row, col) with distinct pairs (sgl.adjacency_edges), its row_ptr, the mirror index (position of
    (cols[e], rows[e])), the table of (c + 1e-10)^-1/2 for every possible degree — the host expression of sgl.norm_csr, so the
    device values carry its bits — and the 64-edge chunks of the base rows.  ValueError for a list that is not such a base,
    WhisprRecHipError for a shape the library refuses."""
    import numpy as np
    from .sgl import degree_scale
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    n_nodes, E = int(n_nodes), int(rows.size)
    if cols.size != E:
        raise ValueError("rows and cols must have one length")
    abi.check_size(abi.lib().wr_sgl_views_workspace_bytes(n_nodes, E), "wr_sgl_views_workspace_bytes")
    if rows.min() < 0 or cols.min() < 0 or rows.max() >= n_nodes or cols.max() >= n_nodes:
        raise ValueError("node id outside [0, n_nodes)")
    keys = rows * n_nodes + cols
    if E > 1 and not np.all(keys[1:] > keys[:-1]):
        raise ValueError("the base edge list must be sorted by (row, col) and hold every pair once")
    mkeys = cols * n_nodes + rows
    mirror = np.minimum(np.searchsorted(keys, mkeys), E - 1)
    if not np.array_equal(keys[mirror], mkeys):
        raise ValueError("the base edge list must be symmetric: (c, r) for every (r, c)")
    cnt = np.bincount(rows, minlength=n_nodes)
    row_ptr = np.zeros(n_nodes + 1, np.int64)
    np.cumsum(cnt, out=row_ptr[1:])
    bchunk_ptr, bchunk_row = spmm_chunks(row_ptr, SGL_VIEW_BASE_CHUNK)
    per = np.bincount(bchunk_row.numpy(), minlength=n_nodes)
    row_first_chunk = np.zeros(n_nodes + 1, np.int64)
    np.cumsum(per, out=row_first_chunk[1:])
    dis_tab = degree_scale(np.arange(int(cnt.max()) + 1, dtype=np.int64))

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to(device)

    return SglViewsBase(n_nodes=n_nodes, n_edges=E, device=torch.device(device), rows=up(rows, np.int32), cols=up(cols, np.int32),
                        mirror=up(mirror, np.int32), row_ptr=up(row_ptr, np.int64), bchunk_ptr=bchunk_ptr.to(device),
                        n_bchunks=int(bchunk_row.numel()), row_first_chunk=up(row_first_chunk, np.int64),
                        dis_tab=up(dis_tab, np.float32))


class _SglViewBuild:
    """One view between its two device phases: count (flags, per-chunk counts, scans, row_ptr, chunk counts) and, once the
    sizes are on the host, fill.  `meta` holds the six numbers fill needs, on the device."""

    def __init__(self, base, kind, n_select, seed, stream_ids):
        if kind not in SGL_VIEW_KINDS:
            raise ValueError("kind must be 'ED' or 'ND' (got %r)" % (kind,))
        ids = [int(s) for s in stream_ids]
        if len(ids) != (1 if kind == "ED" else 2):
            raise ValueError("ED takes one stream id (edges), ND two (row nodes, column nodes)")
        self.base = b = base
        dev, L, M = b.device, abi.lib(), (1 << 64) - 1
        nbytes = abi.check_size(L.wr_sgl_views_workspace_bytes(b.n_nodes, b.n_edges), "wr_sgl_views_workspace_bytes")
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)
        cnt = torch.empty((2, b.n_bchunks), dtype=torch.int32, device=dev)
        abi.check(L.wr_sgl_view_count(SGL_VIEW_KINDS[kind], _p(b.rows), _p(b.cols), _p(b.mirror), b.n_edges, b.n_nodes,
                                      _p(b.bchunk_ptr), b.n_bchunks, int(n_select), int(seed) & M, ids[0] & M, ids[-1] & M,
                                      _p(cnt[0]), _p(cnt[1]), _p(self.err), _p(self.ws), nbytes, _stream()), "wr_sgl_view_count")
        self.scan = torch.zeros((2, b.n_bchunks + 1), dtype=torch.int64, device=dev)
        self.scan[:, 1:].copy_(torch.cumsum(cnt, 1, dtype=torch.int64))
        self.row_ptr = torch.empty((2, b.n_nodes + 1), dtype=torch.int64, device=dev)
        abi.check(L.wr_sgl_view_rows(_p(b.row_first_chunk), b.n_nodes, b.n_bchunks, _p(self.scan[0]), _p(self.scan[1]),
                                     _p(self.row_ptr[0]), _p(self.row_ptr[1]), _stream()), "wr_sgl_view_rows")
        self.chunks = [_chunks_count(self.row_ptr[d]) for d in (0, 1)]
        self.meta = torch.cat([self.scan[:, -1], self.chunks[0][0][-1:], self.chunks[1][0][-1:],
                               self.chunks[0][1].to(torch.int64), self.chunks[1][1].to(torch.int64), self.err.to(torch.int64)])

    META = 7

    def fill(self, meta, chunk_tables=True):
        """meta: the META numbers of self.meta on the host -> per direction (row_ptr, col, val[, chunk_ptr, chunk_row])"""
        b, dev = self.base, self.base.device
        nnz, n_chunks, max_per = meta[0:2], meta[2:4], meta[4:6]
        if meta[6]:
            raise abi.WhisprRecHipError("wr_sgl_view_count: the base arrays contradict their contract (err_word %d)" % meta[6])
        col = [torch.empty(n, dtype=torch.int32, device=dev) for n in nnz]
        val = [torch.empty(n, dtype=torch.float32, device=dev) for n in nnz]
        abi.check(abi.lib().wr_sgl_view_fill(_p(b.rows), _p(b.cols), _p(b.mirror), b.n_edges, b.n_nodes, _p(b.bchunk_ptr),
                                             b.n_bchunks, _p(self.scan[0]), _p(self.scan[1]), _p(self.row_ptr[0]), _p(b.dis_tab),
                                             b.dis_tab.numel(), _p(col[0]) if nnz[0] else None, _p(val[0]) if nnz[0] else None,
                                             nnz[0], _p(col[1]) if nnz[1] else None, _p(val[1]) if nnz[1] else None, nnz[1],
                                             _p(self.err), _p(self.ws), self.ws.numel(), _stream()), "wr_sgl_view_fill")
        out = []
        for d in (0, 1):
            part = (self.row_ptr[d], col[d], val[d])
            if chunk_tables:
                part += _chunks_fill(self.row_ptr[d], self.chunks[d][0], n_chunks[d], max_per[d])
            out.append(part)
        return out


def sgl_views_build(base, kind, specs, seed, chunk_tables=True, err_words=None):
    """Several views of one base with ONE read-back: specs = [(n_keep_or_n_drop, stream_ids), ...] -> per view
    [forward, transposed], each (row_ptr, col, val, chunk_ptr, chunk_row) on the device (chunk_row carries ``_wr_levels``)."""
    builds = [_SglViewBuild(base, kind, n, seed, ids) for n, ids in specs]
    meta = torch.cat([v.meta for v in builds]).tolist()          # the one device-to-host read: sizes of every array
    K = _SglViewBuild.META
    out = [v.fill(meta[i * K:(i + 1) * K], chunk_tables) for i, v in enumerate(builds)]
    if err_words is not None:        # the fill launches' own bits (8, 16: unreachable for scans of the same flags) for who asks
        err_words.extend(v.err for v in builds)
    return out


def sgl_view(base, kind, n_keep_or_n_drop, seed, stream_ids):
    """One view of the device base (wr_sgl_view_*): kind 'ED' keeps the n_keep edges e with perm(e) < n_keep, kind 'ND' drops
    the n_drop row nodes and the n_drop column nodes with perm(v) < n_drop (stream_ids: one id for ED, (rows, cols) for ND;
    perm = oracle.epoch_permutation_at(., n, seed, stream id)).  Returns the device triples (row_ptr int64, col int32, val
    fp32) of the view and of its transpose — bitwise sgl.norm_csr / sgl.transpose_csr of the same kept set."""
    (fwd, bwd), = sgl_views_build(base, kind, [(n_keep_or_n_drop, stream_ids)], seed, chunk_tables=False)
    return fwd, bwd


class HybridSpmm:
    """Normalised-adjacency product with the dense head of the item popularity on the matrix cores (wr_spmm_mfma.hip) and
    the rest on the chunked CSR kernels.  Built once per graph from the symmetric bipartite CSR of LightGCN
    (reference src/models/general/LightGCN.py:54-121: nodes 0..n_users-1 are users, the others items).  Head = the items
    rated by at least `min_density` of the users (at most `max_head`, rounded up to a multiple of 64: two 32-row tiles).  ``enabled`` is False when the graph
    has no such items, no more users than one K split, or nothing but head items — then use spmm_csr_chunked.  The dense tiles
    multiply their zero entries too: a non-finite value in a user row reaches every head item (0 x inf), which the CSR kernels
    would not do; padding columns and rows are masked in the kernel."""

    def __init__(self, row_ptr, col, val, n_users, n_items, device, min_density=0.12, max_head=512, k_split=128):
        import numpy as np
        rp, col, val = np.asarray(row_ptr, np.int64), np.asarray(col, np.int64), np.asarray(val, np.float32)
        nU, nI = int(n_users), int(n_items)
        N = nU + nI
        deg = np.diff(rp)
        order = np.argsort(-deg[nU:], kind="stable")
        n_head = int((deg[nU:] >= min_density * nU).sum())
        H = min((n_head + 63) // 64 * 64, int(max_head) // 64 * 64, nI // 64 * 64)
        # the head-item tiles split K = all users over several workgroups: with no more users than one split holds there is
        # nothing to split (and nothing to gain on so small a graph): CSR kernels only
        self.enabled = H >= 64 and n_head >= 16 and nU > int(k_split)
        self.n_nodes, self.device = N, device
        if not self.enabled:
            return
        head_nodes = nU + order[:H]
        pos_of = np.full(N, -1, np.int64)
        pos_of[head_nodes] = np.arange(H)
        rows = np.repeat(np.arange(N), deg)
        user_head = (rows < nU) & (pos_of[col] >= 0)
        nU_pad = (nU + 31) // 32 * 32
        Dn = np.zeros((nU_pad, H), np.float32)
        Dn[rows[user_head], pos_of[col[user_head]]] = val[user_head]
        self.head_nnz = int(user_head.sum())
        self.density = self.head_nnz / float(nU * H)
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device)
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
        # user-side tiles: 32 users x K = H head items (one split)
        self.u_tiles = nU_pad // 32
        self.u_A = f32(Dn.reshape(self.u_tiles, 32, H).transpose(0, 2, 1))            # [tile][k][32]
        self.u_K = H
        self.u_cols = i32(head_nodes)
        u_rows = np.arange(nU_pad)
        u_rows[nU:] = -1
        self.u_rows = i32(u_rows)
        # item-side tiles: 32 head items x K = all users, K cut into splits of k_split columns
        self.k_split = int(k_split)
        K2 = (nU + self.k_split - 1) // self.k_split * self.k_split
        Dk = np.zeros((K2, H), np.float32)
        Dk[:nU] = Dn[:nU]                                                               # A[h, u] = A[u, h]
        self.i_tiles = H // 32
        self.i_A = f32(Dk.reshape(K2, self.i_tiles, 32).transpose(1, 0, 2))            # [tile][k = user][32 head items]
        self.i_K = K2
        i_cols = np.arange(K2)
        i_cols[nU:] = -1                                                                # padding columns: masked in the kernel (exact zeros)
        self.i_cols = i32(i_cols)
        self.i_rows = i32(head_nodes)
        # CSR part: everything but the (user, head item) entries and the head items' rows
        keep = ~(user_head | (pos_of[rows] >= 0))
        if not keep.any():
            self.enabled = False        # every item is a head item: no CSR part to carry the user rows' layer sum
            return
        r_deg = np.bincount(rows[keep], minlength=N)
        r_rp = np.zeros(N + 1, np.int64)
        np.cumsum(r_deg, out=r_rp[1:])
        cptr, crow = spmm_chunks(r_rp)
        self.chunk_ptr, self.chunk_row = cptr.to(device), crow.to(device)
        self.col, self.val = i32(col[keep]), f32(val[keep])
        mode = np.zeros(N, np.int8)
        mode[:nU] = 1
        mode[head_nodes] = 2
        self.row_mode = torch.from_numpy(mode).to(device)
        self.n_head, self.H = n_head, H
        self._partials = {}

    def apply(self, X, Y=None, acc=None):
        """Y = A X (and acc += Y); X [n_nodes, D] fp32"""
        L = abi.lib()
        _req(X, torch.float32, "X", 2)
        N, D = X.shape
        if Y is None:
            Y = torch.empty_like(X)
        pt = self._partials.get(D)
        if pt is None:
            nb = abi.check_size(L.wr_spmm_dense_partials_bytes(self.i_tiles, self.i_K, self.k_split, D), "wr_spmm_dense_partials_bytes")
            pt = (torch.empty(max(nb // 4, 4), dtype=torch.float32, device=X.device),
                  torch.empty((self.chunk_row.numel(), D), dtype=torch.float32, device=X.device))
            self._partials[D] = pt
        # one launch for both tile groups: user rows get their dense part in Y (the CSR kernels then add the rest and the
        # layer sum); head item rows are complete on the matrix cores (K = all users, split over workgroups)
        g0 = abi.DenseGroup(_p(self.u_A), _p(self.u_cols), _p(self.u_rows), None, self.u_K, self.u_K, self.u_tiles)
        g1 = abi.DenseGroup(_p(self.i_A), _p(self.i_cols), _p(self.i_rows), _p(pt[0]), self.i_K, self.k_split, self.i_tiles)
        abi.check(L.wr_spmm_dense_tiles(ctypes.addressof(g0), ctypes.addressof(g1), _p(X), N, D, _p(Y), _p(acc), _stream()),
                  "wr_spmm_dense_tiles")
        abi.check(L.wr_spmm_csr_chunked_modes(N, self.chunk_row.numel(), _p(self.chunk_ptr), _p(self.chunk_row), _p(self.col),
                                              _p(self.val), _p(X), D, _p(Y), _p(acc), _p(pt[1]), _p(self.row_mode), _stream()),
                  "wr_spmm_csr_chunked_modes")
        return Y


def axpy(y, x, alpha, overwrite=False):
    abi.check(abi.lib().wr_axpy(_p(_req(y, torch.float32, "y")), _p(_req(x, torch.float32, "x")), y.numel(), alpha,
                                1 if overwrite else 0, _stream()), "wr_axpy")
    return y


def lightgcn_step(user_tab, item_tab, csr, n_layers, u, p, n, reg_weight, trusted=False):
    """LightGCN.predict + backward in one native call (wr_lightgcn_step): -> (loss (1,), gradient [n_users + n_items, D], error
    flag tensor or None).  csr = (chunk_ptr, chunk_row, col, val) of the normalised adjacency on the device."""
    cptr, crow, col, val = csr
    u, p, n = _idx64(u, "u"), _idx64(p, "p"), _idx64(n, "n")
    _req(user_tab, torch.float32, "user_tab", 2)
    _req(item_tab, torch.float32, "item_tab", 2)
    dev, D, B = user_tab.device, user_tab.shape[1], u.numel()
    L = abi.lib()
    nbytes = abi.check_size(L.wr_lightgcn_step_workspace_bytes(user_tab.shape[0], item_tab.shape[0], D, crow.numel(), B),
                            "wr_lightgcn_step_workspace_bytes")
    ws = workspace(dev, "lgcn_step").get(nbytes)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    grad = torch.empty(user_tab.shape[0] + item_tab.shape[0], D, dtype=torch.float32, device=dev)
    err = None if trusted else torch.zeros(1, dtype=torch.int32, device=dev)
    abi.check(L.wr_lightgcn_step(_p(user_tab), _p(item_tab), user_tab.shape[0], item_tab.shape[0], D, crow.numel(), _p(cptr),
                                 _p(crow), _p(col), _p(val), spmm_levels_of(crow), int(n_layers), _p(u), _p(p), _p(n), B,
                                 float(reg_weight), 1 if trusted else 0, _p(loss), _p(grad), _p(err), _p(ws), ws.numel(),
                                 _stream()), "wr_lightgcn_step")
    return loss, grad, err


def embloss_grad(user_tab, item_tab, plan, k, sq3, reg_weight, grad_user, grad_item):
    """EmbLoss backward for batch k of a plan (wr_embloss_grad): adds into grad_user / grad_item, no host sync."""
    off = k * plan.batch_size
    abi.check(abi.lib().wr_embloss_grad(_p(user_tab), _p(item_tab), user_tab.shape[1], plan.tu.data_ptr() + 4 * off,
                                        plan.oc_item.data_ptr() + 8 * off, plan.oc_src.data_ptr() + 8 * off,
                                        plan.batch_len(k), _p(sq3), reg_weight, _p(grad_user), _p(grad_item), _stream()),
              "wr_embloss_grad")


def lightgcn_loss(user_all, item_all, user_ego, item_ego, u, p, n, reg_weight):
    """LightGCN.predict's per-batch tail (wr_lightgcn_loss): -> (loss tensor of shape (1,), sq3 tensor of the three EmbLoss
    sums of squares)"""
    u, p, n = _idx64(u, "u"), _idx64(p, "p"), _idx64(n, "n")
    for t, nm in ((user_all, "user_all"), (item_all, "item_all"), (user_ego, "user_ego"), (item_ego, "item_ego")):
        _req(t, torch.float32, nm, 2)
    B, D = u.numel(), user_all.shape[1]
    dev = user_all.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    sq3 = torch.empty(3, dtype=torch.float32, device=dev)
    L = abi.lib()
    ws = workspace(dev, "lgcn_loss").get(abi.check_size(L.wr_lightgcn_loss_workspace_bytes(B), "wr_lightgcn_loss_workspace_bytes"))
    abi.check(L.wr_lightgcn_loss(_p(user_all), _p(item_all), _p(user_ego), _p(item_ego), user_all.shape[0], item_all.shape[0], D,
                                 _p(u), _p(p), _p(n), B, float(reg_weight), _p(loss), _p(sq3), _p(ws), ws.numel(), _stream()),
              "wr_lightgcn_loss")
    return loss, sq3


def embloss_sumsq(user_tab, item_tab, u, p, n):
    u, p, n = _idx64(u, "u"), _idx64(p, "p"), _idx64(n, "n")
    B, D = u.numel(), user_tab.shape[1]
    out = torch.empty(3, dtype=torch.float32, device=user_tab.device)
    ws = workspace(user_tab.device, "embloss").get(((B + 15) // 16 + 1) * 12 + 256)
    abi.check(abi.lib().wr_embloss_sumsq(_p(user_tab), _p(item_tab), D, _p(u), _p(p), _p(n), B, _p(out), _p(ws),
                                         ws.numel(), _stream()), "wr_embloss_sumsq")
    return out
