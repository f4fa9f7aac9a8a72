// host_api.hip -- the host layer: the context and its scratch buffers, the
// launch helpers and the C ABI (include/capnp_packed.h).  Included last by
// packed_codec.hip, after every kernel: one translation unit.
#include "carve.hip"  // Carve: a scratch layout written once (counted, then carved)

struct HostPipe;  // host_pipe.hip: staging of the host-memory forms

// A device buffer of the context, allocated on first use (valid when zeroed:
// the context is calloc'ed).  reserve() grows one on demand, reserve_fixed()
// allocates one of a fixed size; cpk_ctx_destroy frees the ones its list names.
struct DevBuf {
  uint64_t *p;
  uint64_t cap;  // entries (reserve); unused by the fixed-size ones
};

struct cpk_ctx_s {
  int device;
  int cus;
  DevBuf status;          // look-back words
  uint32_t *tickets;      // cpk::kTkWords words: per-XCD counters, plan ticket, error bits
  int encoder;            // 0: single pass (encode_sp.hip); 4: size + emit passes; 5: by piece size
  int sp_form;            // the single pass's form: 0 by density, 1 dense, 2 sparse (CPK_SP_FORM)
  int decoder;            // 2: record index (decode_v2.hip); 1: block map (decode_kernel); 3: by density
  DevBuf sp_status;       // single pass: look-back word per piece
  uint32_t sp_epoch;      //   launch epoch tagging the look-back words, 1..65535
  DevBuf sp_desc;         //   message batches: piece descriptors | segment tables
  DevBuf e4_bv;           // encoder v4: per 64-word step its run boundaries, members, heads (kE4RowBytes each)
  HostPipe *pipe;         // cpk_encode_host / cpk_decode_host staging (lazy)
  DevBuf ss_buf;          // parallel stream decode scratch (stream_split.hip)
  DevBuf ms_buf;          // cpk_decode_message_stream: the frame chain's entries (messages) and result row
  DevBuf ems_buf;         // cpk_encode_message_stream: the result row | the pieces' word offsets
  DevBuf rm_buf;          // cpk_read_message: piece word offsets | piece ends | statuses (fixed size)
  DevBuf fl_buf;          // cpk_decode_batch of a few large pieces: boundaries found [33] (fixed size)
  uint64_t *probe_pin;    // host read-backs of a few device words (read_words): pinned [8] (lazy)
  DevBuf rm_copy;         // cpk_read_message_host, one-wave path: the packed bytes on the device (fixed size)
  uint64_t small_seq;     // the one-launch host paths' completion flag values (small_wait)
  uint64_t small_fallbacks;  // small_wait calls whose flag was unset even after a stream sync (lost flags)
  uint64_t small_timeouts;   // small_wait calls that waited past 5 ms (late launches included)
  DevBuf sp_units;        // single pass, pieces over one chunk: unit counts | starts | block sums | unit table
  uint64_t rm_mw_max;     // cpk_read_message[_host]: streams under it by one workgroup (<= kRmMwMax)
  int e4_order;           // cpk_encode_messages' two passes, segments largest first: 1 both passes,
                          // 2 the emit pass only, 0 neither (CPK_E4_ORDER)
  int size_form;          // cpk_packed_size_batch: 0 by piece size, 1 chunk parallel, 2 wave per piece (CPK_SIZE_FORM)
  int usize_form;         // cpk_unpacked_size_batch: 0 by piece size, 1 block map, 2 wave per piece (CPK_USIZE_FORM)
  int at_form;            // cpk_encode_batch_at: 0 by density, 1 dense, 2 sparse (CPK_AT_FORM)
  DevBuf at_buf;          // cpk_encode_batch_at with groups: the groups' first units [ng + 1] | the pieces' groups [n]
  int msg_at_form;        // cpk_encode_messages_at: 0 by segment size, 1 wave, 2 placed (CPK_MSG_AT_FORM)
  DevBuf mat_buf;         // cpk_encode_messages_at: what its two forms pass between their kernels (mat_scratch)
  // CPK_HOST_TRACE=1 (read at creation): host wall time of the one-message
  // host paths (cpk_encode_host[_gather], cpk_read_message_host) by phase,
  // summed per context and printed to stderr by cpk_ctx_destroy
  bool trace;
  double tr_us[8];
  uint64_t tr_n[8];
};
// the phases (write: staging in, enqueues, waits, staging out; read: same)
enum { kTrWIn, kTrWLaunch, kTrWWait, kTrWOut, kTrRIn, kTrRLaunch, kTrRWait, kTrROut };
struct TrClock {
  cpk_ctx c;
  std::chrono::steady_clock::time_point t;
  explicit TrClock(cpk_ctx ctx) : c(ctx) {
    if (c->trace) t = std::chrono::steady_clock::now();
  }
  void mark(int k) {
    if (!c->trace) return;
    const auto n = std::chrono::steady_clock::now();
    c->tr_us[k] += std::chrono::duration<double, std::micro>(n - t).count();
    ++c->tr_n[k];
    t = n;
  }
};

namespace {
int hip_ok(hipError_t e) { return e == hipSuccess ? CPK_OK : CPK_EDEVICE; }

// hipMemsetAsync for the device entry points, safe under graph capture.  A
// memset captured into a graph is a memset node, and the HIP runtime this was
// found on leaves part of such a node's range unset from the second launch of
// the graph on (2,176 bytes: the last 544 keep their old values; a plain HIP
// program shows it, tests/test_gpu_graph_replay.py found it: ticket counters
// and a counting sort's histogram not cleared, then stores out of bounds).
// So while `s` is being captured the bytes are set by a kernel node instead;
// an uncaptured call is the hipMemsetAsync it always was.  p: 4-byte aligned
// in every use here (any other pointer takes hipMemsetAsync).
__global__ void fill_kernel(uint8_t *p, uint32_t v4, uint64_t bytes) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t nw = bytes / 4;
  for (uint64_t k = i; k < nw; k += step) reinterpret_cast<uint32_t *>(p)[k] = v4;
  if (i < (bytes & 3)) p[4 * nw + i] = (uint8_t)v4;
}
// Whether work enqueued on `s` is being captured into a graph.  A status query
// that fails is taken for a capture: what the callers do for one (a kernel for
// a memset node, a clear ahead of the look-back, no read-back) is never wrong.
bool stream_captured(hipStream_t s) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
}
hipError_t fill_async(void *p, int value, size_t bytes, hipStream_t s) {
  if (!stream_captured(s) || ((uintptr_t)p & 3) || bytes == 0) return hipMemsetAsync(p, value, bytes, s);
  const uint64_t blocks = (bytes / 4 + 255) / 256;
  hipLaunchKernelGGL(fill_kernel, dim3((unsigned)(blocks < 1 ? 1 : blocks > 1024 ? 1024 : blocks)), dim3(256), 0, s,
                     (uint8_t *)p, 0x01010101u * (uint32_t)(value & 0xff), (uint64_t)bytes);
  return hipGetLastError();
}

struct DeviceGuard {
  int prev;
  explicit DeviceGuard(int d) {
    hipGetDevice(&prev);
    if (prev != d) hipSetDevice(d);
  }
  ~DeviceGuard() {
    int cur;
    hipGetDevice(&cur);
    if (cur != prev) hipSetDevice(prev);
  }
};

// `probe` of cpk_decode_batch and cpk_unpacked_size_batch: a batch of <= 32
// pieces may read its extent back (one sync) to give a few large pieces a
// faster path, never while the stream is being captured.  The host forms pass
// false: they know the sizes, and their two-slot pipeline never blocks on it.
bool may_probe(cpk_ctx ctx, uint32_t n, void *stream) {
  if (n > 32 || !ctx) return false;
  DeviceGuard g(ctx->device);
  return !stream_captured((hipStream_t)stream);
}

// order[0..n) = 0..n-1 by size class, largest first (cpk::ord_*); hist:
// kOrdClasses u32 of scratch
void ord_launch(const uint64_t *words, uint32_t n, uint32_t *hist, uint32_t *order, hipStream_t s,
                const uint64_t *swo = nullptr) {
  const unsigned tb = 256, tg = (n + tb - 1) / tb;
  (void)fill_async(hist, 0, 4 * cpk::kOrdClasses, s);
  hipLaunchKernelGGL(cpk::ord_hist_kernel, dim3(tg), dim3(tb), 0, s, words, n, hist, swo);
  hipLaunchKernelGGL(cpk::ord_scan_kernel, dim3(1), dim3(64), 0, s, hist);
  hipLaunchKernelGGL(cpk::ord_scatter_kernel, dim3(tg), dim3(tb), 0, s, words, n, hist, order, swo);
}

// out[0..n] = the exclusive scan of in[0..n), out[n] the total (in may be
// out: each thread reads its entries before it writes them); bsum:
// scan_blocks(n) words of scratch
uint32_t scan_blocks(uint64_t n) { return (uint32_t)((n + cpk::kE4ScanBlock - 1) / cpk::kE4ScanBlock); }
void scan_launch(const uint64_t *in, uint32_t n, uint64_t *bsum, uint64_t *out, hipStream_t s) {
  const uint32_t nb = scan_blocks(n);
  hipLaunchKernelGGL(cpk::e4_scan_reduce, dim3(nb), dim3(cpk::kE4ScanThreads), 0, s, in, n, bsum);
  hipLaunchKernelGGL(cpk::e4_scan_top, dim3(1), dim3(cpk::kE4ScanThreads), 0, s, bsum, nb);
  hipLaunchKernelGGL(cpk::e4_scan_down, dim3(nb), dim3(cpk::kE4ScanThreads), 0, s, in, n, (const uint64_t *)bsum,
                     out);
}

// the decoders' ticket counters (one per XCD) back to zero
hipError_t dec_tickets_reset(cpk_ctx ctx, hipStream_t s) {
  return fill_async(ctx->tickets + cpk::kTkDec, 0, 8 * cpk::kTkStride * 4, s);
}

// every ticket counter and the plan ticket (the words below the error word)
// back to zero: before the two passes and the size calls
hipError_t enc_tickets_reset(cpk_ctx ctx, hipStream_t s) {
  return fill_async(ctx->tickets, 0, cpk::kTkErr * 4, s);
}

// the two passes' grid: persistent blocks of kE4Waves waves, a wave per piece
unsigned e4_grid(cpk_ctx ctx, uint32_t n) {
  const unsigned grid = (unsigned)(8 * ctx->cus), want = (n + cpk::kE4Waves - 1) / cpk::kE4Waves;
  return grid > want ? want : grid;
}

// The front half of the block map over `reach` bytes in nb blocks
// (stream_split.hip): every block's walks, the groups' and the stream's
// chains, the blocks' first records.  swo / n: the stream's pieces, where the
// caller knows them.
int ss_map_launch(cpk_ctx ctx, const uint8_t *pk, uint64_t reach, const uint64_t *swo, uint32_t n, uint64_t nb,
                  const cpk::SsBufs &B, hipStream_t s) {
  using namespace cpk;
  const uint64_t ng = (nb + kSsGroup - 1) / kSsGroup;
  if (fill_async(B.N2, 0, 4 * nb, s) != hipSuccess || fill_async(B.flag, 0, 8, s) != hipSuccess ||
      dec_tickets_reset(ctx, s) != hipSuccess)
    return CPK_EDEVICE;
  const unsigned tb = 256, gb = (unsigned)((nb + tb - 1) / tb);
  hipLaunchKernelGGL(ss_scan_kernel, dim3((unsigned)ng), dim3(kSsThreads), kSsLds, s, pk, reach, swo, n, nb, B);
  hipLaunchKernelGGL(ss_group_kernel, dim3((unsigned)ng), dim3(64), 0, s, pk, nb, B);
  hipLaunchKernelGGL(ss_top_kernel, dim3(1), dim3(64), 0, s, pk, nb, B);
  hipLaunchKernelGGL(ss_cut_kernel, dim3(gb), dim3(tb), 0, s, nb, B);
  return CPK_OK;
}

// Room for `need` entries in b: a new allocation of max(floor, need + need / 4)
// entries when it has fewer, of bytes(entries) bytes (8 each when null).
// *grew tells the caller that the buffer is new (its contents undefined).
// After a failed allocation the buffer is empty: p null, cap 0.
int reserve(DevBuf &b, uint64_t need, uint64_t floor = 0, uint64_t (*bytes)(uint64_t) = nullptr,
            bool *grew = nullptr) {
  if (b.p && need <= b.cap) return CPK_OK;
  if (b.p) hipFree(b.p);
  b.p = nullptr;
  b.cap = 0;
  const uint64_t cap = need < floor ? floor : need + need / 4;
  if (hipMalloc(&b.p, bytes ? bytes(cap) : cap * 8) != hipSuccess) {
    b.p = nullptr;
    return CPK_ENOMEM;
  }
  b.cap = cap;
  if (grew) *grew = true;
  return CPK_OK;
}
// a buffer of a fixed size, allocated by the first call
int reserve_fixed(DevBuf &b, uint64_t bytes) {
  if (b.p || hipMalloc(&b.p, bytes) == hipSuccess) return CPK_OK;
  b.p = nullptr;
  return CPK_ENOMEM;
}
// Room in b for a layout, then its pointers: `layout(Carve &)` is the list of
// take() calls, run once counting and once over the buffer.  fixed: one of
// the fixed-size buffers (reserve_fixed), its layout the same for every call.
template <class Layout>
int carve_reserve(DevBuf &b, uint64_t floor, Layout layout, bool fixed = false) {
  Carve count;
  layout(count);
  if (int rc = fixed ? reserve_fixed(b, count.n * 8) : reserve(b, count.n, floor)) return rc;
  Carve c(b.p);
  layout(c);
  return CPK_OK;
}

// sizes [n] | the scan's block sums: the scratch of a size pass and its scan
// (e4_encode, cpk_packed_size_batch)
int sizes_scratch(cpk_ctx ctx, uint32_t n, uint64_t *&sizes, uint64_t *&bsum) {
  return carve_reserve(ctx->status, 1024, [&](Carve &c) {
    sizes = c.take(n);
    bsum = c.take(scan_blocks(n) + 1);
  });
}
}  // namespace

static int decode_batch_impl(cpk_ctx ctx, const void *d_packed, const uint64_t *d_in_off, const uint64_t *d_swo,
                             uint32_t n, void *d_out, int32_t *d_status, void *stream, bool probe);
static int unpacked_size_impl(cpk_ctx ctx, const void *d_packed, const uint64_t *d_in_off, uint32_t n,
                              uint64_t *d_swo, int32_t *d_status, void *stream, bool probe, const uint64_t *h_off);

// The end of a one-launch small path (rm_small_kernel, sp_small_kernel):
// its kernel writes seq to *flag (pinned host memory) after all its other
// writes, so the host reads its results once the flag turns -- without the
// stream synchronisation's wait for the kernel's completion signal.  Past a
// bound (the kernel is slow or faulted) the stream synchronisation decides.
// Returns 0 or nonzero like hipStreamSynchronize.
// The flag word is cleared by small_arm before the launch (it is pinned
// memory other calls use for other data) and its values carry a tag no
// offset or size the slot held can equal.
constexpr uint64_t kSmallTag = 0x5ea1ull << 48;
static uint64_t small_arm(cpk_ctx ctx, uint64_t *flag) {
  __atomic_store_n(flag, 0ull, __ATOMIC_RELEASE);
  return kSmallTag | (++ctx->small_seq & ((1ull << 48) - 1));
}
static int small_wait(cpk_ctx ctx, hipStream_t s, const uint64_t *flag, uint64_t seq) {
  const auto t0 = std::chrono::steady_clock::now();
  for (uint32_t i = 1;; ++i) {
    if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) return 0;
    __builtin_ia32_pause();
    if ((i & 1023) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(5)) break;
  }
  // A late launch (a busy GPU, queueing behind other streams, the first
  // module load) also gets here: the stream synchronisation decides.  Only a
  // flag still unset after it -- a kernel that completed without writing it,
  // a device-side bug -- is counted (cpk_ctx_small_fallbacks); a lost flag
  // would otherwise only cost 5 ms per call and pass every test.
  ++ctx->small_timeouts;
  if (hipStreamSynchronize(s) != hipSuccess) return 1;
  if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) return 0;
  ++ctx->small_fallbacks;
  return 1;
}
#include "host_pipe.hip"

extern "C" {

int cpk_abi_version(void) { return CPK_ABI_VERSION; }

#ifdef CPK_PHASE_STATS
// diagnostic builds only: read and clear the per-phase cycle sums
int cpk_debug_phase_stats(unsigned long long *host64) {
  if (hipMemcpyFromSymbol(host64, HIP_SYMBOL(cpk::g_phase), 64 * 8) != hipSuccess) return CPK_EDEVICE;
  unsigned long long z[64] = {0};
  return hipMemcpyToSymbol(HIP_SYMBOL(cpk::g_phase), z, sizeof z) == hipSuccess ? CPK_OK : CPK_EDEVICE;
}
#endif

const char *cpk_status_string(int s) {
  switch (s) {
    case CPK_OK: return "ok";
    case CPK_EINVAL: return "invalid argument / misaligned piece";
    case CPK_ETRUNC: return "premature end of packed input";
    case CPK_EOVERRUN: return "packed run past the end of the piece";
    case CPK_ETRAILING: return "piece filled before the end of its packed bytes";
    case CPK_EFRAME: return "invalid segment table";
    case CPK_ENOMEM: return "out of device memory";
    case CPK_EDEVICE: return "HIP runtime error";
    case CPK_EUNSUPPORTED: return "piece not supported by this build";
    default: return "unknown status";
  }
}

uint64_t cpk_packed_bound(uint64_t words) { return 8 * words + 2 * ((words + 1) / 2); }

uint64_t cpk_batch_packed_capacity(const uint64_t *h_swo, uint32_t n) {
  uint64_t s = 0;
  for (uint32_t i = 0; i < n; ++i) s += cpk_packed_bound(h_swo[i + 1] - h_swo[i]);
  return s + 16;
}

int cpk_ctx_create(int device, cpk_ctx *out) {
  if (!out) return CPK_EINVAL;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count)
    return CPK_EDEVICE;
  DeviceGuard g(device);
  cpk_ctx c = (cpk_ctx)calloc(1, sizeof(cpk_ctx_s));
  if (!c) return CPK_ENOMEM;
  c->device = device;
  {
    // Encoders: the single pass (encode_sp.hip) for batches of like-sized
    // pieces of 4 Ki words and more (3.65 against 5.06 ms per 131,072
    // config-2 pieces of 8 Ki words; 3.96 against 5.50 ms for 16,384 of
    // 64 Ki words), the two passes (encode_v4.hip) for mixed sizes and
    // message batches; chosen on the device (e4_gate_kernel) among the
    // batches sp_takes admits.  CPK_ENCODER=0 / 4 force one of them.
    const char *e = getenv("CPK_ENCODER");
    c->encoder = (e && e[0] == '4') ? 4 : (e && e[0] == '0') ? 0 : 5;
    // CPK_SP_FORM=dense / sparse forces the single pass's form where the
    // gate picks the single pass (A/B of the density threshold)
    const char *f = getenv("CPK_SP_FORM");
    c->sp_form = (f && f[0] == 'd') ? 1 : (f && f[0] == 's') ? 2 : 0;
    // CPK_DECODER=1 selects the block-map decoder, 2 the record-index one
    const char *d = getenv("CPK_DECODER");
    c->decoder = (d && d[0] == '2') ? 2 : (d && d[0] == '1') ? 1 : 3;
    const char *t = getenv("CPK_HOST_TRACE");
    c->trace = t && t[0] == '1';
    // (CPK_RM_MW_MAX_KB: A/B of the one-workgroup reader's upper bound)
    const char *m = getenv("CPK_RM_MW_MAX_KB");
    c->rm_mw_max = m ? (uint64_t)atoll(m) << 10 : 0;
    const char *o = getenv("CPK_E4_ORDER");
    c->e4_order = o ? atoi(o) : 1;
    // CPK_SIZE_FORM=chunk / wave forces the size query's form (A/B of its gate)
    const char *z = getenv("CPK_SIZE_FORM");
    c->size_form = (z && z[0] == 'c') ? 1 : (z && z[0] == 'w') ? 2 : 0;
    // CPK_USIZE_FORM=1 / 2 forces the unpacked-size query's form: the block
    // map for every piece it can take, a wave per piece (A/B of its threshold)
    const char *u = getenv("CPK_USIZE_FORM");
    c->usize_form = (u && u[0] == '1') ? 1 : (u && u[0] == '2') ? 2 : 0;
    // CPK_AT_FORM=dense / sparse forces the placed encoder's form (A/B of its gate)
    const char *a = getenv("CPK_AT_FORM");
    c->at_form = (a && a[0] == 'd') ? 1 : (a && a[0] == 's') ? 2 : 0;
    // CPK_MSG_AT_FORM=wave / place forces cpk_encode_messages_at's form (A/B of its gate)
    const char *ma = getenv("CPK_MSG_AT_FORM");
    c->msg_at_form = (ma && ma[0] == 'w') ? 1 : (ma && ma[0] == 'p') ? 2 : 0;
  }
  if (hipDeviceGetAttribute(&c->cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess)
    c->cus = 256;
  if (hipMalloc(&c->tickets, cpk::kTkWords * 4) != hipSuccess ||
      hipMemset(c->tickets, 0, cpk::kTkWords * 4) != hipSuccess) {
    free(c);
    return CPK_ENOMEM;
  }
  // the kernels' dynamic LDS, above the 64 KiB default for some: set here,
  // with the context's device current (the attribute is per device).  The
  // library is built for gfx950 only (160 KiB of LDS per CU): each request
  // is checked against that at compile time, so a refused attribute is a
  // runtime/driver failure, reported as CPK_EDEVICE
  constexpr uint32_t kGfx950Lds = 160 * 1024;
  static_assert(cpk::kDecLds <= kGfx950Lds && cpk::SpLay<cpk::SpDense>::kLds <= kGfx950Lds &&
                    cpk::kSpSmallLds <= kGfx950Lds && cpk::kMwLds <= kGfx950Lds && cpk::kSsLds <= kGfx950Lds,
                "a kernel's dynamic LDS exceeds gfx950's 160 KiB");
  const struct {
    const void *f;
    uint32_t bytes;
  } lds[] = {{(const void *)cpk::decode_kernel<false>, cpk::kDecLds},
             {(const void *)cpk::decode_kernel<true>, cpk::kDecLds},
             {(const void *)cpk::decode_kernel<false, true>, cpk::kDecLds},
             {(const void *)cpk::decode_kernel<true, true>, cpk::kDecLds},
             {(const void *)cpk::sp_encode_kernel<true>, cpk::SpLay<cpk::SpDense>::kLds},
             {(const void *)cpk::sp_encode_kernel<false>, cpk::SpLay<cpk::SpDense>::kLds},
             {(const void *)cpk::sp_place_kernel<cpk::SpDense>, cpk::SpLay<cpk::SpDense>::kLds},
             {(const void *)cpk::sp_small_kernel, cpk::kSpSmallLds},
             {(const void *)cpk::rm_mw_kernel, cpk::kMwLds},
             {(const void *)cpk::stream_mw_kernel, cpk::kMwLds},
             {(const void *)cpk::ss_scan_kernel, cpk::kSsLds}};
  for (const auto &k : lds)
    if (hipFuncSetAttribute(k.f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.bytes) != hipSuccess) {
      hipFree(c->tickets);
      free(c);
      return CPK_EDEVICE;
    }
  *out = c;
  return CPK_OK;
}

void cpk_ctx_destroy(cpk_ctx ctx) {
  if (!ctx) return;
  DeviceGuard g(ctx->device);
  if (ctx->trace) {
    static const char *nm[8] = {"write staging in", "write enqueue", "write wait", "write staging out",
                                "read staging in", "read enqueue", "read wait", "read staging out"};
    for (int k = 0; k < 8; ++k)
      if (ctx->tr_n[k])
        fprintf(stderr, "cpk host trace: %-18s %8llu marks %12.1f us total\n", nm[k],
                (unsigned long long)ctx->tr_n[k], ctx->tr_us[k]);
  }
  // (every DevBuf member: a new one is added here)
  for (DevBuf *b : {&ctx->status, &ctx->sp_status, &ctx->sp_desc, &ctx->sp_units, &ctx->e4_bv, &ctx->ss_buf,
                    &ctx->ms_buf, &ctx->ems_buf, &ctx->rm_buf, &ctx->fl_buf, &ctx->rm_copy, &ctx->at_buf, &ctx->mat_buf})
    if (b->p) hipFree(b->p);
  if (ctx->tickets) hipFree(ctx->tickets);
  if (ctx->probe_pin) hipHostFree(ctx->probe_pin);
  pipe_destroy(ctx->pipe);
  free(ctx);
}

int cpk_ctx_device(cpk_ctx ctx) { return ctx ? ctx->device : -1; }
uint64_t cpk_ctx_small_fallbacks(cpk_ctx ctx) { return ctx ? ctx->small_fallbacks : 0; }
int cpk_ctx_dense_windows(cpk_ctx ctx, void *stream, uint64_t *serial, uint64_t *given_back) {
  if (!ctx || !serial || !given_back) return CPK_EINVAL;
  if (!cpk::kDecCnt) return CPK_EUNSUPPORTED;  // (counted by the diagnostics build only)
  DeviceGuard g(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  uint32_t c[2] = {0, 0};
  if (hipMemcpyAsync(c, ctx->tickets + cpk::kTkDec + 1, 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return CPK_EDEVICE;
  *serial = c[0];
  *given_back = c[1];
  return CPK_OK;
}

// The device words at src[0..k) (k <= 8) on the host, after the work already
// on stream s: one small kernel writes them to the context's pinned words.
static int read_words(cpk_ctx ctx, hipStream_t s, std::initializer_list<const uint64_t *> src, uint64_t *dst) {
  if (!ctx->probe_pin && hipHostMalloc((void **)&ctx->probe_pin, 8 * 8, hipHostMallocDefault) != hipSuccess) {
    ctx->probe_pin = nullptr;
    return CPK_ENOMEM;
  }
  cpk::Gather8 g = {};
  uint32_t k = 0;
  for (const uint64_t *p : src) g.p[k++] = p;
  hipLaunchKernelGGL(cpk::gather8_kernel, dim3(1), dim3(64), 0, s, g, k, ctx->probe_pin);
  if (hipStreamSynchronize(s) != hipSuccess) return CPK_EDEVICE;
  for (uint32_t i = 0; i < k; ++i) dst[i] = ctx->probe_pin[i];
  return CPK_OK;
}

// Single-pass encoder (encode_sp.hip): one launch, the look-back words
// epoch-tagged (cleared only when the epoch wraps or the array grows, and by
// every launch captured into a graph, as a node of that graph: sp_plan).  Work
// is ticketed per 8192-word chunk of a piece (a unit); a batch whose pieces
// may be larger than one chunk (the hint) first gets its unit table (three
// small kernels and the e4 scan, no host sync: the unit count stays on the
// device).  sp_takes screens which batches it takes; cpk_encode_batch lets
// the device choose by the piece sizes (e4_gate_kernel).

// A bound on the units of n pieces (0: every piece is one unit): from the
// hint, no piece being over it; with no hint from the batch's word total,
// which bounds every piece.  Over 2^32 units: unsupported.
static uint64_t sp_unit_bound(uint64_t n, uint64_t hint, uint64_t total = 0) {
  constexpr uint64_t chunk = 64ull * cpk::kSpCS;
  if (hint) return hint <= chunk ? 0 : n * ((hint + chunk - 1) / chunk);
  return total <= chunk ? 0 : n + total / chunk + 1;
}
// ... of a batch on the device: with no hint its word total is read back,
// synchronising the stream
static int sp_batch_unit_bound(cpk_ctx ctx, const uint64_t *d_swo, uint32_t n, uint64_t hint, hipStream_t s,
                               uint64_t &ub) {
  uint64_t ends[2] = {0, 0};
  if (!hint)
    if (int rc = read_words(ctx, s, {d_swo, d_swo + n}, ends)) return rc;
  ub = sp_unit_bound(n, hint, ends[1] - ends[0]);
  return CPK_OK;
}
// whether the single pass is enqueued at all (for the device to choose): a
// size hint, and a unit table of bounded size for pieces over one chunk (a
// loose hint would otherwise size it for nothing)
static bool sp_takes(cpk_ctx ctx, uint32_t n, uint64_t max_seg_words) {
  if (ctx->encoder == 0) return true;  // (CPK_ENCODER=0: single pass for every batch)
  return ctx->encoder != 4 && max_seg_words != 0 && sp_unit_bound(n, max_seg_words) <= (1ull << 25);
}

// What a launch ticketed by units needs (sp_encode_kernel, sz_chunk_kernel;
// both see the same epoch tagging, which SpHandover's no-hang argument
// assumes): ucap look-back words and as many run-state words, tagged with a
// new epoch, and the unit table when pieces may exceed one chunk.
struct SpPlan {
  uint64_t ucap;                  // units at most
  uint64_t *status, *ustate;      // look-back words [ucap] | run-state words [ucap]
  uint32_t epoch;                 // 1..65535; kSpEpochCaptured for a launch being captured into a graph
  const uint64_t *utab, *nunits;  // the unit table and its count on the device; null: every piece one unit
};
// the epoch of every captured launch: the tag of a cleared word, so only words
// the launch's own graph wrote after its own clear can carry a flag under it
constexpr uint32_t kSpEpochCaptured = 0;
// `units`: a bound on the batch's units when its pieces may exceed one chunk
// (0: every piece is one unit).  pdesc, hint: as the kernels take them.
static int sp_plan(cpk_ctx ctx, const uint64_t *d_swo, const uint64_t *pdesc, uint32_t n, uint64_t hint,
                   uint64_t units, hipStream_t s, SpPlan &P) {
  P.ucap = units ? units : n;
  // (a grown array's words are undefined, and a look-back polls them:
  // cleared below, as when the epoch wraps)
  bool fresh = false;
  if (int rc = reserve(ctx->sp_status, 2 * P.ucap, 8192, nullptr, &fresh)) return rc;
  // A launch captured into a graph runs again at every replay with the
  // arguments it was captured with, the epoch among them: the words the last
  // replay left would be valid for the next.  So a captured launch takes no
  // epoch from the counter: it is tagged kSpEpochCaptured, which no eager
  // launch ever draws (the counter runs 1..65535), and the clear of the words
  // it polls is enqueued ahead of it, a node of the graph.
  const bool captured = stream_captured(s);
  if (!captured && ++ctx->sp_epoch > 0xffffu) {
    ctx->sp_epoch = 1;
    fresh = true;
  }
  const uint64_t clear = fresh ? ctx->sp_status.cap : captured ? 2 * P.ucap : 0;
  if (clear && fill_async(ctx->sp_status.p, 0, clear * 8, s) != hipSuccess) return CPK_EDEVICE;
  P.status = ctx->sp_status.p;
  P.ustate = P.status + P.ucap;
  P.epoch = captured ? kSpEpochCaptured : ctx->sp_epoch;
  P.utab = P.nunits = nullptr;
  if (!units) return CPK_OK;
  // unit counts -> starts (e4 scan) -> unit table
  uint64_t *ucnt, *ustart, *bsum, *tab;
  if (int rc = carve_reserve(ctx->sp_units, 0, [&](Carve &c) {
        ucnt = c.take(n);
        ustart = c.take((uint64_t)n + 1);
        bsum = c.take(scan_blocks(n) + 1);
        tab = c.take(units);
      }))
    return rc;
  const unsigned tb = 256, tg = (n + tb - 1) / tb;
  hipLaunchKernelGGL(cpk::sp_units_count_kernel, dim3(tg), dim3(tb), 0, s, d_swo, pdesc, n, hint, ucnt);
  scan_launch(ucnt, n, bsum, ustart, s);
  hipLaunchKernelGGL(cpk::sp_units_fill_kernel, dim3(tg), dim3(tb), 0, s, (const uint64_t *)ustart, n, tab);
  P.utab = tab;
  P.nunits = ustart + n;
  return CPK_OK;
}
// the persistent grid of a plan's kernel: wpe workgroups per CU, never more than the units
static unsigned sp_grid(cpk_ctx ctx, int wpe, const SpPlan &P) {
  const uint64_t grid = (uint64_t)wpe * ctx->cus;
  return (unsigned)(grid > P.ucap ? P.ucap : grid);
}

int sp_launch(cpk_ctx ctx, const void *d_in, const uint64_t *d_swo, const uint64_t *pdesc,
              const uint64_t *tin, uint32_t n, uint64_t hint, void *d_out, uint64_t *d_out_off,
              hipStream_t s, bool gated = false, uint64_t units = 0, uint64_t out_cap = ~0ull) {
  SpPlan P;
  if (int rc = sp_plan(ctx, d_swo, pdesc, n, hint, units, s, P)) return rc;
  // (gated: the ticket was set by e4_gate_kernel -- exhausted unless the
  // batch is the single pass's)
  if (!gated && fill_async(ctx->tickets + cpk::kTkPlan, 0, 4, s) != hipSuccess) return CPK_EDEVICE;
  // (gated: both forms enqueued, the one the gate did not pick returns at once)
  const uint32_t *pick = gated ? ctx->tickets + cpk::kTkGate + cpk::kGateSparse : nullptr;
  // (tin: the tables' words of a message batch, the output bound before them)
  const uint64_t *bound = tin ? tin - 1 : nullptr;
  auto launch = [&](auto kernel, int wpe, uint32_t lds, uint32_t form) {
    hipLaunchKernelGGL(kernel, dim3(sp_grid(ctx, wpe, P)), dim3(cpk::kSpThreads), lds, s, (const uint64_t *)d_in,
                       d_swo, pdesc, tin, n, (uint8_t *)d_out, d_out_off, P.status, P.epoch,
                       ctx->tickets + cpk::kTkPlan, P.utab, P.nunits, P.ustate, hint, ctx->tickets + cpk::kTkErr, bound,
                       pick, form, out_cap);
  };
  launch(pdesc ? cpk::sp_encode_kernel<true> : cpk::sp_encode_kernel<false>, cpk::SpDense::kWpe,
         cpk::SpLay<cpk::SpDense>::kLds, 0u);
  if (gated && !pdesc)
    launch(cpk::sp_encode_kernel<false, cpk::SpSparse>, cpk::SpSparse::kWpe, cpk::SpLay<cpk::SpSparse>::kLds, 1u);
  return hip_ok(hipGetLastError());
}

// The size pass's rows for the emit pass (kE4RowBytes per 64-word step):
// `stride` rows per piece from the hint when they fit in 4 GiB, else packed
// by word offset (stride 0: the batch's word count is read back, synchronising
// the stream)
static int e4_rows(cpk_ctx ctx, const uint64_t *d_swo, uint32_t n, uint64_t hint, hipStream_t s,
                   uint64_t &stride) {
  stride = hint ? (hint + 63) / 64 : 0;
  if (stride && stride > cpk::kE4MaxRows / (n ? n : 1)) stride = 0;  // (no overflow)
  uint64_t rows;
  if (stride) {
    rows = (uint64_t)(n ? n : 1) * stride;
  } else {
    uint64_t ends[2];
    int rc = read_words(ctx, s, {d_swo, d_swo + n}, ends);
    if (rc) return rc;
    rows = (ends[1] - ends[0]) / 64 + n + 1;
  }
  return reserve(ctx->e4_bv, rows, 0, [](uint64_t cap) { return cap * cpk::kE4RowBytes; });
}

// Encoder v4 (encode_v4.hip): size pass, scan, emit pass.  Pieces of any
// size; a piece over the hint is reported (output undefined).  The size pass
// leaves each 64-word step's run boundaries for the emit pass: `stride` rows
// per piece from the hint, or packed by word offset when there is no hint (the
// batch's word count is then read back, synchronising the stream).
// The two passes' kernels, each launched from here alone.  rows: whether the
// size pass keeps its boundary rows (e4_rows, `stride`) for an emit pass;
// skip: a device gate's word (nonzero: the other form took the batch), or
// null; order: the pieces largest first, or null; err: where a piece over the
// hint is reported, null: the context's error word (cpk_ctx_take_error).
static void e4_size_launch(cpk_ctx ctx, const void *d_in, const uint64_t *d_swo, uint32_t n, uint64_t hint,
                           uint64_t *sizes, bool rows, uint64_t stride, const uint32_t *skip,
                           const uint32_t *order, hipStream_t s, uint32_t *err = nullptr) {
  hipLaunchKernelGGL(rows ? cpk::e4_size_kernel<true> : cpk::e4_size_kernel<false>, dim3(e4_grid(ctx, n)),
                     dim3(cpk::kE4Threads), 0, s, (const uint64_t *)d_in, d_swo, n, sizes,
                     ctx->tickets + cpk::kTkEnc, hint, err ? err : ctx->tickets + cpk::kTkErr,
                     rows ? ctx->e4_bv.p : (uint64_t *)nullptr, rows ? stride : (uint64_t)0, skip, order);
}
// (off: the pieces' output offsets; sizes: the size pass's; ends: an end per
// piece in place of out_cap, a piece past its own skipped without a report)
static void e4_emit_launch(cpk_ctx ctx, const void *d_in, const uint64_t *d_swo, uint32_t n, const uint64_t *off,
                           const uint64_t *sizes, uint64_t stride, const uint32_t *skip, const uint32_t *order,
                           void *d_out, uint64_t out_cap, hipStream_t s, const uint64_t *ends = nullptr) {
  auto launch = [&](auto kernel, auto cap) {
    hipLaunchKernelGGL(kernel, dim3(e4_grid(ctx, n)), dim3(cpk::kE4Threads), cpk::kE4Lds, s, (const uint64_t *)d_in,
                       d_swo, n, off, (uint8_t *)d_out, ctx->tickets + cpk::kTkDec, (const uint64_t *)ctx->e4_bv.p,
                       stride, skip, sizes, cap, ctx->tickets + cpk::kTkErr, order);
  };
  if (ends)
    launch(cpk::e4_emit_kernel<true>, ends);
  else
    launch(cpk::e4_emit_kernel<false>, out_cap);
}

// Arms a device gate over the piece sizes (e4_gate_kernel, sz_gate_kernel):
// the gate block's min / max words preset and e4_minmax_kernel over the
// batch; sampled: it also samples the words at d_in (their counts are
// cleared first).  -> the samples taken
static int gate_arm(cpk_ctx ctx, const uint64_t *d_swo, uint32_t n, bool sampled, const void *d_in, hipStream_t s,
                    uint32_t &samples) {
  uint32_t *mm = ctx->tickets + cpk::kTkGate;
  if (fill_async(mm + cpk::kGateMin, 0xff, 4, s) != hipSuccess ||
      fill_async(mm + cpk::kGateMax, 0, 4, s) != hipSuccess)
    return CPK_EDEVICE;
  if (sampled && (fill_async(mm + cpk::kGateZero, 0, 4, s) != hipSuccess ||
                  fill_async(mm + cpk::kGateBytes, 0, 4, s) != hipSuccess))
    return CPK_EDEVICE;
  const unsigned mg = n < 256u * 256u ? (unsigned)((n + 255) / 256) : 256u;
  hipLaunchKernelGGL(cpk::e4_minmax_kernel, dim3(mg), dim3(256), 0, s, d_swo, n, mm,
                     sampled ? (const uint64_t *)d_in : (const uint64_t *)nullptr);
  samples = mg * 256u;
  return CPK_OK;
}

int e4_encode(cpk_ctx ctx, const void *d_in, const uint64_t *d_swo, uint32_t n, uint64_t hint,
              void *d_out, uint64_t *d_out_off, hipStream_t s, bool gate = false, uint64_t out_cap = ~0ull) {
  uint64_t *sizes, *bsum, stride;
  if (int rc = sizes_scratch(ctx, n, sizes, bsum)) return rc;
  if (int rc = e4_rows(ctx, d_swo, n, hint, s, stride)) return rc;
  if (enc_tickets_reset(ctx, s) != hipSuccess) return CPK_EDEVICE;
  const uint32_t *skip = nullptr;
  if (gate) {
    // which encoder takes the batch, decided on the device from the piece
    // sizes (no host sync): the other's tickets are exhausted, so its
    // kernels return at once (the scans then write offsets the single pass
    // overwrites)
    uint32_t samples;
    if (int rc = gate_arm(ctx, d_swo, n, true, d_in, s, samples)) return rc;
    hipLaunchKernelGGL(cpk::e4_gate_kernel, dim3(1), dim3(64), 0, s, ctx->tickets, samples, (uint32_t)ctx->sp_form,
                       d_swo, n);
    skip = ctx->tickets + cpk::kTkGate + cpk::kGatePick;
  }
  e4_size_launch(ctx, d_in, d_swo, n, hint, sizes, true, stride, skip, nullptr, s);
  scan_launch(sizes, n, bsum, d_out_off, s);
  e4_emit_launch(ctx, d_in, d_swo, n, d_out_off, sizes, stride, skip, nullptr, d_out, out_cap, s);
  return hip_ok(hipGetLastError());
}

// The front half of the two passes over a message batch: d_out_off = the
// pieces' packed offsets in message order (a table per message, then its
// segments).  rows: an emit pass follows -- the size pass keeps its boundary
// rows (e4_rows, which without a hint synchronises the stream) and the
// segments' output offsets get room.  Segments are taken largest first (a
// wave takes a whole segment, and a 256 KiB one taken last kept the rest of
// the chip idle behind it): by CPK_E4_ORDER=1 in both passes, =2 in the emit
// pass only.  d_out_off null: the pieces' sizes alone, no offsets (the caller
// places the messages itself); skip, err: as e4_size_launch takes them.
struct MsgPass {
  uint64_t *ssize, *tsize;  // the segments' and the tables' packed sizes
  uint64_t *soff;           // the segments' output offsets, for msg_table_emit_kernel to write (rows only)
  const uint32_t *order;    // the segments largest first, or null
  uint64_t stride;          // e4_rows (rows only)
};
static int msg_front(cpk_ctx ctx, const void *d_in, const uint64_t *d_swo, uint32_t nseg,
                     const uint64_t *d_msg_seg_off, uint32_t nm, uint64_t hint, uint64_t *d_out_off, hipStream_t s,
                     bool rows, MsgPass &M, const uint32_t *skip = nullptr, uint32_t *err = nullptr) {
  const uint64_t np = (uint64_t)nm + nseg;
  uint64_t *comb, *bsum;
  uint32_t *sord, *shist;
  if (int rc = carve_reserve(ctx->status, 1024, [&](Carve &c) {
        M.ssize = c.take(nseg);
        M.tsize = c.take(nm);
        comb = c.take(np);  // both, in message order
        M.soff = rows ? c.take(nseg) : nullptr;
        bsum = c.take(scan_blocks(np) + 1);
        sord = c.take32(nseg);
        shist = c.take32(cpk::kOrdClasses);
        // (the order has always been given nseg / 2 + 1 entries, one more than
        // an even nseg needs: kept, so the size asked for is what it was)
        const uint64_t spare = nseg & 1 ? 0 : 1;
        c.take(spare);
      }))
    return rc;
  M.stride = 0;
  if (rows)
    if (int rc = e4_rows(ctx, d_swo, nseg, hint, s, M.stride)) return rc;
  if (enc_tickets_reset(ctx, s) != hipSuccess) return CPK_EDEVICE;
  M.order = nullptr;
  if (nseg && (ctx->e4_order == 1 || (rows && ctx->e4_order))) {
    ord_launch(nullptr, nseg, shist, sord, s, d_swo);
    M.order = sord;
  }
  if (nseg)
    e4_size_launch(ctx, d_in, d_swo, nseg, hint, M.ssize, rows, M.stride, skip,
                   ctx->e4_order == 1 ? M.order : nullptr, s, err);
  // the tables, sized as msg_table_emit_kernel builds them
  const unsigned tb = 256, tg = (nm + tb - 1) / tb;
  hipLaunchKernelGGL(cpk::msg_table_size_kernel, dim3(tg), dim3(tb), 0, s, d_swo, d_msg_seg_off, nm, M.tsize);
  if (!d_out_off) return CPK_OK;
  hipLaunchKernelGGL(cpk::msg_interleave_kernel, dim3(tg), dim3(tb), 0, s, d_msg_seg_off, nm,
                     (const uint64_t *)M.tsize, (const uint64_t *)M.ssize, comb);
  scan_launch(comb, (uint32_t)np, bsum, d_out_off, s);
  return CPK_OK;
}

int cpk_encode_messages(cpk_ctx ctx, const void *d_in, const uint64_t *d_swo, uint32_t nseg,
                        const uint64_t *d_msg_seg_off, uint32_t nm, uint64_t max_seg_words,
                        void *d_out, uint64_t *d_out_off, void *stream) {
  return cpk_encode_messages_cap(ctx, d_in, d_swo, nseg, d_msg_seg_off, nm, max_seg_words, d_out, ~0ull,
                                 d_out_off, stream);
}
int cpk_encode_messages_cap(cpk_ctx ctx, const void *d_in, const uint64_t *d_swo, uint32_t nseg,
                            const uint64_t *d_msg_seg_off, uint32_t nm, uint64_t max_seg_words,
                            void *d_out, uint64_t out_cap, uint64_t *d_out_off, void *stream) {
  if (!ctx || !d_out_off || (nm && !d_msg_seg_off) || (nseg && !d_swo)) return CPK_EINVAL;
  if (((uintptr_t)d_out & 15) || ((uintptr_t)d_in & 7)) return CPK_EINVAL;
  if (max_seg_words == 0) return CPK_EINVAL;  // (a bound is needed for the step rows)
  DeviceGuard g(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  if (nm == 0) return hip_ok(fill_async(d_out_off, 0, 8, s));
  const uint64_t np = (uint64_t)nm + nseg;  // pieces: a table per message + the segments
  if (np > 0xffffffffull) return CPK_EINVAL;
  if (ctx->encoder == 0 || (ctx->encoder != 4 && np <= 1024)) {
    // single pass (forced, or a small batch -- one SerializePacked.write:
    // two launches instead of the two passes' nine; a large batch of mixed
    // sizes takes the two passes, faster there): piece descriptors in
    // message order + the tables' words
    if (int rc = reserve(ctx->sp_desc, 2 * np + (uint64_t)nseg / 2 + nm + 2)) return rc;
    // pdesc[2 np] | output bound | tables
    uint64_t *pdesc = ctx->sp_desc.p, *tbuf = ctx->sp_desc.p + 2 * np + 1;
    const unsigned tb = 256, tg = (nm + tb - 1) / tb;
    hipLaunchKernelGGL(cpk::sp_msg_prep_kernel, dim3(tg), dim3(tb), 0, s, d_swo, d_msg_seg_off, nm, pdesc,
                       tbuf, tbuf - 1);
    // (tables are at most 257 words: the segments' hint bounds the units)
    const uint64_t ub = sp_unit_bound(np, max_seg_words);
    if (ub > 0xffffffffull) return CPK_EUNSUPPORTED;
    return sp_launch(ctx, d_in, nullptr, pdesc, tbuf, (uint32_t)np, max_seg_words, d_out, d_out_off, s, false, ub,
                     out_cap);
  }
  MsgPass M;
  if (int rc = msg_front(ctx, d_in, d_swo, nseg, d_msg_seg_off, nm, max_seg_words, d_out_off, s, true, M)) return rc;
  const unsigned tb = 256, tg = (nm + tb - 1) / tb;
  hipLaunchKernelGGL(cpk::msg_table_emit_kernel, dim3(tg), dim3(tb), 0, s, d_swo, d_msg_seg_off, nm,
                     (const uint64_t *)d_out_off, M.soff, (uint8_t *)d_out, (const uint64_t *)M.tsize, out_cap,
                     ctx->tickets + cpk::kTkErr);
  if (nseg) e4_emit_launch(ctx, d_in, d_swo, nseg, M.soff, M.ssize, M.stride, nullptr, M.order, d_out, out_cap, s);
  return hip_ok(hipGetLastError());
}

int cpk_encode_batch(cpk_ctx ctx, const void *d_in, const uint64_t *d_swo, uint32_t n,
                     uint64_t max_seg_words, void *d_out, uint64_t *d_out_off, void *stream) {
  return cpk_encode_batch_cap(ctx, d_in, d_swo, n, max_seg_words, d_out, ~0ull, d_out_off, stream);
}
int cpk_encode_batch_cap(cpk_ctx ctx, const void *d_in, const uint64_t *d_swo, uint32_t n,
                         uint64_t max_seg_words, void *d_out, uint64_t out_cap, uint64_t *d_out_off,
                         void *stream) {
  if (!ctx || (!d_swo && n) || !d_out_off) return CPK_EINVAL;
  if (((uintptr_t)d_out & 15) || ((uintptr_t)d_in & 7)) return CPK_EINVAL;
  DeviceGuard g(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) return hip_ok(fill_async(d_out_off, 0, 8, s));
  if (!sp_takes(ctx, n, max_seg_words))
    return e4_encode(ctx, d_in, d_swo, n, max_seg_words, d_out, d_out_off, s, false, out_cap);
  if (ctx->encoder == 0) {
    // (forced single pass: pieces of any size, several units for a large one)
    uint64_t ub;
    if (int rc = sp_batch_unit_bound(ctx, d_swo, n, max_seg_words, s, ub)) return rc;
    if (ub > 0xffffffffull) return CPK_EUNSUPPORTED;
    return sp_launch(ctx, d_in, d_swo, nullptr, nullptr, n, max_seg_words, d_out, d_out_off, s, false, ub,
                     out_cap);
  }
  // by piece size: both enqueued, the device picks one (e4_gate_kernel);
  // pieces over one chunk go to the single pass as several units
  int rc = e4_encode(ctx, d_in, d_swo, n, max_seg_words, d_out, d_out_off, s, true, out_cap);
  if (rc) return rc;
  return sp_launch(ctx, d_in, d_swo, nullptr, nullptr, n, max_seg_words, d_out, d_out_off, s, true,
                   sp_unit_bound(n, max_seg_words), out_cap);
}

// ---- exact packed sizes without encoding (encode_size.hip) -----------------
// Two forms, both enqueued for the device to choose (sz_gate_kernel): the
// chunk-parallel one over the single pass's plan (sp_plan), and the two
// passes' wave-per-piece size walk without boundary rows.
int cpk_packed_size_batch(cpk_ctx ctx, const void *d_in, const uint64_t *d_swo, uint32_t n,
                          uint64_t max_seg_words, uint64_t *d_out_off, void *stream) {
  if (!ctx || (!d_swo && n) || !d_out_off) return CPK_EINVAL;
  if ((uintptr_t)d_in & 7) return CPK_EINVAL;
  DeviceGuard g(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) return hip_ok(fill_async(d_out_off, 0, 8, s));
  // a bound on the batch's 8192-word units (0: every piece is one): from the
  // hint, or from the batch's word count read back (synchronising the stream,
  // as cpk_encode_batch without a hint).  The chunk-parallel form is enqueued
  // (for the device to choose) when its unit table stays of bounded size.
  uint64_t ub;
  if (int rc = sp_batch_unit_bound(ctx, d_swo, n, max_seg_words, s, ub)) return rc;
  const bool can_chunk = ctx->size_form != 2 && ub <= (1ull << 25);
  uint64_t *sizes, *bsum;
  if (int rc = sizes_scratch(ctx, n, sizes, bsum)) return rc;
  if (enc_tickets_reset(ctx, s) != hipSuccess || fill_async(sizes, 0, (uint64_t)n * 8, s) != hipSuccess)
    return CPK_EDEVICE;
  // the form, decided on the device from the piece sizes (no host sync, no
  // sample of the words)
  uint32_t samples;
  if (int rc = gate_arm(ctx, d_swo, n, false, nullptr, s, samples)) return rc;
  hipLaunchKernelGGL(cpk::sz_gate_kernel, dim3(1), dim3(64), 0, s, ctx->tickets, d_swo, n, can_chunk ? 1u : 0u,
                     (uint32_t)ctx->size_form);
  if (can_chunk) {
    SpPlan P;
    if (int rc = sp_plan(ctx, d_swo, nullptr, n, max_seg_words, ub, s, P)) return rc;
    hipLaunchKernelGGL(cpk::sz_chunk_kernel, dim3(sp_grid(ctx, cpk::kSzWpe, P)), dim3(cpk::kSpThreads), 0, s,
                       (const uint64_t *)d_in, d_swo, n, (unsigned long long *)sizes, ctx->tickets + cpk::kTkPlan,
                       P.utab, P.nunits, P.ustate, P.epoch, max_seg_words, ctx->tickets + cpk::kTkErr);
  }
  e4_size_launch(ctx, d_in, d_swo, n, max_seg_words, sizes, false, 0, ctx->tickets + cpk::kTkGate + cpk::kGatePick,
                 nullptr, s);
  scan_launch(sizes, n, bsum, d_out_off, s);
  return hip_ok(hipGetLastError());
}

int cpk_packed_size_messages(cpk_ctx ctx, const void *d_in, const uint64_t *d_swo, uint32_t nseg,
                             const uint64_t *d_msg_seg_off, uint32_t nm, uint64_t max_seg_words,
                             uint64_t *d_out_off, void *stream) {
  if (!ctx || !d_out_off || (nm && !d_msg_seg_off) || (nseg && !d_swo)) return CPK_EINVAL;
  if ((uintptr_t)d_in & 7) return CPK_EINVAL;
  DeviceGuard g(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  if (nm == 0) return hip_ok(fill_async(d_out_off, 0, 8, s));
  const uint64_t np = (uint64_t)nm + nseg;  // pieces: a table per message + the segments
  if (np > 0xffffffffull) return CPK_EINVAL;
  MsgPass M;
  if (int rc = msg_front(ctx, d_in, d_swo, nseg, d_msg_seg_off, nm, max_seg_words, d_out_off, s, false, M)) return rc;
  return hip_ok(hipGetLastError());
}

// ---- encode to caller-given offsets (encode_at.hip, encode_msg_at.hip) ------
// The placed single pass over A's pieces and groups: the single pass's plan
// (sp_plan: units, status words, epoch; ub: sp_unit_bound's units), the piece
// -> group map (at_prep_kernel) and both forms of sp_place_kernel, enqueued for
// the device to choose: tickets[kTkGate + kGateSparse] names the one that runs
// (0 dense, 1 sparse), left there by the caller's gate (at_gate_kernel over
// e4_minmax_kernel's sample), which has been enqueued.
static int at_place_launch(cpk_ctx ctx, cpk::AtArgs A, const uint64_t *d_grp_piece_off, uint64_t max_seg_words,
                           uint64_t ub, hipStream_t s) {
  const uint32_t n = A.n, ng = A.ng;
  const uint64_t *d_swo = A.swo;
  const unsigned tb = 256, gg = (ng + tb - 1) / tb;
  SpPlan P;
  if (int rc = sp_plan(ctx, d_swo, nullptr, n, max_seg_words, ub, s, P)) return rc;
  // (the pieces' first units: the scan the unit table was filled from)
  const uint64_t *ustart = P.nunits ? P.nunits - n : nullptr;
  uint64_t *gfirst = nullptr;
  uint32_t *pgrp = nullptr;
  if (d_grp_piece_off) {
    if (int rc = carve_reserve(ctx->at_buf, 1024, [&](Carve &c) {
          gfirst = c.take((uint64_t)ng + 1);
          pgrp = c.take32(n);
        }))
      return rc;
    if (fill_async(pgrp, 0xff, (uint64_t)n * 4, s) != hipSuccess) return CPK_EDEVICE;
  }
  hipLaunchKernelGGL(cpk::at_prep_kernel, dim3(gg), dim3(tb), 0, s, A, d_grp_piece_off, ustart, pgrp, gfirst);
  A.pgrp = pgrp;
  A.gfirst = d_grp_piece_off ? gfirst : ustart;  // (a piece its own group: its first unit)
  const uint32_t *pick = ctx->tickets + cpk::kTkGate + cpk::kGateSparse;
  auto launch = [&](auto kernel, int wpe, uint32_t lds, uint32_t form) {
    hipLaunchKernelGGL(kernel, dim3(sp_grid(ctx, wpe, P)), dim3(cpk::kSpThreads), lds, s, A, P.status, P.epoch,
                       ctx->tickets + cpk::kTkPlan, P.utab, P.nunits, P.ustate, max_seg_words,
                       ctx->tickets + cpk::kTkErr, pick, form);
  };
  launch(cpk::sp_place_kernel<cpk::SpDense>, cpk::SpDense::kWpe, cpk::SpLay<cpk::SpDense>::kLds, 0u);
  launch(cpk::sp_place_kernel<cpk::SpSparse>, cpk::SpSparse::kWpe, cpk::SpLay<cpk::SpSparse>::kLds, 1u);
  return hip_ok(hipGetLastError());
}

int cpk_encode_batch_at(cpk_ctx ctx, const void *d_in, const uint64_t *d_swo, uint32_t n, uint64_t max_seg_words,
                        const uint64_t *d_grp_piece_off, uint32_t ng, void *d_out, uint64_t out_cap,
                        const uint64_t *d_dst_off, const uint64_t *d_dst_cap, uint64_t *d_piece_off,
                        uint64_t *d_grp_len, int32_t *d_status, void *stream) {
  if (!ctx || (!d_swo && n) || (!d_piece_off && n)) return CPK_EINVAL;
  if (ng && (!d_dst_off || !d_grp_len || !d_status || !d_out)) return CPK_EINVAL;
  if (d_grp_piece_off ? (ng == 0 && n != 0) : ng != n) return CPK_EINVAL;
  if (((uintptr_t)d_out & 15) || ((uintptr_t)d_in & 7) || ((uintptr_t)d_status & 3)) return CPK_EINVAL;
  for (const void *q : {(const void *)d_swo, (const void *)d_grp_piece_off, (const void *)d_dst_off,
                        (const void *)d_dst_cap, (const void *)d_piece_off, (const void *)d_grp_len})
    if ((uintptr_t)q & 7) return CPK_EINVAL;
  if (ng == 0) return CPK_OK;
  DeviceGuard g(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  // (no offset or length of a real buffer is near 2^64: the kernels' byte
  // addresses then never wrap)
  if (out_cap > (1ull << 62)) out_cap = 1ull << 62;
  cpk::AtArgs A = {(const uint64_t *)d_in, d_swo,      n,           ng,        (uint8_t *)d_out, out_cap, d_dst_off,
                   d_dst_cap,              nullptr,    nullptr,     d_piece_off, d_grp_len,      d_status};
  const unsigned tb = 256, gg = (ng + tb - 1) / tb;
  if (n == 0) {
    // (groups without pieces: their statuses and lengths)
    hipLaunchKernelGGL(cpk::at_prep_kernel, dim3(gg), dim3(tb), 0, s, A, d_grp_piece_off,
                       (const uint64_t *)nullptr, (uint32_t *)nullptr, (uint64_t *)nullptr);
    return hip_ok(hipGetLastError());
  }
  // a bound on the batch's 8192-word units (0: every piece is one): from the
  // hint; with no hint, or one so loose that the unit table it bounds would
  // pass 2^25 entries, from the batch's word count read back (synchronising
  // the stream, as cpk_encode_batch without a hint)
  uint64_t ub = max_seg_words ? sp_unit_bound(n, max_seg_words) : 0;
  if (!max_seg_words || ub > (1ull << 25))
    if (int rc = sp_batch_unit_bound(ctx, d_swo, n, 0, s, ub)) return rc;
  if (ub > 0xffffffffull) return CPK_EUNSUPPORTED;
  uint32_t samples;
  if (int rc = gate_arm(ctx, d_swo, n, true, d_in, s, samples)) return rc;
  hipLaunchKernelGGL(cpk::at_gate_kernel, dim3(1), dim3(64), 0, s, ctx->tickets, samples, (uint32_t)ctx->at_form);
  return at_place_launch(ctx, A, d_grp_piece_off, max_seg_words, ub, s);
}

int cpk_encode_messages_at(cpk_ctx ctx, const void *d_in, const uint64_t *d_swo, uint32_t nseg,
                           const uint64_t *d_msg_seg_off, uint32_t nm, uint64_t max_seg_words, void *d_out,
                           uint64_t out_cap, const uint64_t *d_dst_off, const uint64_t *d_dst_cap,
                           uint64_t *d_piece_off, uint64_t *d_msg_len, int32_t *d_status, void *stream) {
  using namespace cpk;
  if (!ctx || max_seg_words == 0 || (nseg && !d_swo)) return CPK_EINVAL;
  if (nm && (!d_msg_seg_off || !d_out || !d_dst_off || !d_piece_off || !d_msg_len || !d_status)) return CPK_EINVAL;
  if (((uintptr_t)d_out & 15) || ((uintptr_t)d_in & 7) || ((uintptr_t)d_status & 3)) return CPK_EINVAL;
  for (const void *q : {(const void *)d_swo, (const void *)d_msg_seg_off, (const void *)d_dst_off,
                        (const void *)d_dst_cap, (const void *)d_piece_off, (const void *)d_msg_len})
    if ((uintptr_t)q & 7) return CPK_EINVAL;
  if (nm == 0) return CPK_OK;
  if ((uint64_t)nm + nseg > 0xffffffffull) return CPK_EINVAL;
  DeviceGuard g(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  if (out_cap > (1ull << 62)) out_cap = 1ull << 62;  // (as cpk_encode_batch_at: no byte address wraps)
  // (a segment of 2^31 words or more is refused whatever the bound: a larger
  // bound says no more, and none of the arithmetic below wraps)
  if (max_seg_words >= (1ull << 31)) max_seg_words = (1ull << 31) - 1;
  // What can run, known without a read-back: the two passes when the size
  // pass's rows at max_seg_words stay within their 4 GiB, the placed single
  // pass when its unit table stays within 2^25 entries.  A forced form
  // (CPK_MSG_AT_FORM) is enqueued alone where it can run.
  const bool rows_fit = (max_seg_words + 63) / 64 <= kE4MaxRows / (nseg ? nseg : 1);
  const uint64_t ub = sp_unit_bound(nseg, max_seg_words);
  const bool units_fit = nseg && ub <= (1ull << 25);
  if (!rows_fit && !units_fit) return CPK_EUNSUPPORTED;
  const bool wave = rows_fit && !(ctx->msg_at_form == 2 && units_fit);
  const bool place = units_fit && !(ctx->msg_at_form == 1 && rows_fit);
  MatArgs M = {};
  uint64_t *tsize, *glen, *spoff;
  int32_t *gst;
  uint32_t *err;
  if (int rc = carve_reserve(ctx->mat_buf, 1024, [&](Carve &c) {
        M.send = c.take(nseg);
        M.base = c.take(nm);
        M.cap = c.take(nm);
        tsize = wave ? nullptr : c.take(nm);  // (the wave form's front sizes the tables: msg_front)
        glen = c.take(nm);
        spoff = c.take(nseg);
        gst = reinterpret_cast<int32_t *>(c.take32(nm));
        err = c.take32(1);  // (a sink: written by the size pass, never cleared, never read)
      }))
    return rc;
  // the form: cpk_encode_batch's rule over the segments as pieces, then the
  // placed encoder's density rule, then what was enqueued (mat_pick_kernel)
  if (nseg) {
    uint32_t samples;
    if (int rc = gate_arm(ctx, d_swo, nseg, true, d_in, s, samples)) return rc;
    hipLaunchKernelGGL(e4_gate_kernel, dim3(1), dim3(64), 0, s, ctx->tickets, samples, 0u, d_swo, nseg);
    hipLaunchKernelGGL(at_gate_kernel, dim3(1), dim3(64), 0, s, ctx->tickets, samples, (uint32_t)ctx->at_form);
  }
  const uint32_t *pick = ctx->tickets + kTkGate + kGatePick;
  hipLaunchKernelGGL(mat_pick_kernel, dim3(1), dim3(64), 0, s, ctx->tickets, wave ? 1u : 0u, place ? 1u : 0u);
  const unsigned tb = 256, tg = (nm + tb - 1) / tb;
  MsgPass F = {};
  if (wave) {
    // (a segment over max_seg_words is the message's CPK_EINVAL, not the
    // context's error: the size pass reports it into a word of our own,
    // which nobody reads; a segment of no message keeps offset and end 0 and
    // is not emitted)
    if (int rc = msg_front(ctx, d_in, d_swo, nseg, d_msg_seg_off, nm, max_seg_words, nullptr, s, nseg != 0, F, pick,
                           err))
      return rc;
    M.soff = F.soff;
    if (nseg && (fill_async(M.send, 0, (uint64_t)nseg * 8, s) != hipSuccess ||
                 fill_async(M.soff, 0, (uint64_t)nseg * 8, s) != hipSuccess))
      return CPK_EDEVICE;
    tsize = F.tsize;
  } else {
    hipLaunchKernelGGL(msg_table_size_kernel, dim3(tg), dim3(tb), 0, s, d_swo, d_msg_seg_off, nm, tsize);
  }
  M.mseg = d_msg_seg_off;
  M.tsize = tsize;
  M.ssize = F.ssize;
  M.hint = max_seg_words;
  M.glen = glen;
  M.gst = gst;
  M.spoff = spoff;
  M.pick = pick;
  const AtArgs U = {(const uint64_t *)d_in, d_swo, nseg, nm, (uint8_t *)d_out, out_cap, d_dst_off, d_dst_cap,
                    nullptr, nullptr, d_piece_off, d_msg_len, d_status};
  hipLaunchKernelGGL(mat_slot_kernel, dim3(tg), dim3(tb), 0, s, U, M);
  if (wave && nseg)
    e4_emit_launch(ctx, d_in, d_swo, nseg, M.soff, F.ssize, F.stride, pick, F.order, d_out, out_cap, s, M.send);
  if (place) {
    // the segments as the placed encoder's pieces, a message's as a group,
    // behind the table and into what the table left of the slot
    const AtArgs A = {(const uint64_t *)d_in, d_swo, nseg, nm, (uint8_t *)d_out, out_cap, M.base, M.cap,
                      nullptr, nullptr, spoff, glen, gst};
    if (int rc = at_place_launch(ctx, A, d_msg_seg_off, max_seg_words, ub, s)) return rc;
    hipLaunchKernelGGL(mat_finish_kernel, dim3(tg), dim3(tb), 0, s, U, M);
  }
  return hip_ok(hipGetLastError());
}

int cpk_ctx_take_error(cpk_ctx ctx, void *stream) {
  if (!ctx) return CPK_EINVAL;
  DeviceGuard g(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  uint32_t e = 0;
  if (hipMemcpyAsync(&e, ctx->tickets + cpk::kTkErr, 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return CPK_EDEVICE;
  if (e && fill_async(ctx->tickets + cpk::kTkErr, 0, 4, s) != hipSuccess) return CPK_EDEVICE;
  // kErrHint: a piece over its size hint; kErrWait: a cross-workgroup wait
  // timed out (cannot happen by design: every wave it waits on is resident);
  // kErrCap: packed bytes would have passed the caller's output capacity
  // (nothing was written there: ArrayOutputStream.java:40-42 -> IOException)
  if (!e) return CPK_OK;
  return (e & cpk::kErrWait) ? CPK_EDEVICE : (e & cpk::kErrCap) ? CPK_ENOMEM : CPK_EINVAL;
}

}  // extern "C"
// ---- the decoders' launch layer ---------------------------------------------
namespace {
// which decoder a single-decoder call uses (the record-index one only when
// forced: the by-density choice is made for batches, cpk_decode_batch)
bool dec_v2(cpk_ctx ctx) { return ctx->decoder == 2; }
// the context's choice (dec_v2), the block map, the record index, the block
// map's dense form (decode_kernel<.., true>); the last three in the order of
// the gates' skip words (dec_gate_kernel, dat_gate_kernel) and of kDecForms
enum DecKind { kDecCtx, kDecMap, kDecIndex, kDecDense };
DecKind dec_ctx_kind(cpk_ctx ctx) { return dec_v2(ctx) ? kDecIndex : kDecMap; }
// the shapes a decoder is launched in: batch, stream, batch on a range per piece (decode_at.hip)
enum DecShape { kDecBatch, kDecStream, kDecAt };

// A decoder form, described here alone: its kernel for each shape (all take
// the same arguments), its threads and its dynamic LDS.  A new form is a new
// DecKind and its row here (and its word of the gates' skip words).
struct DecForm {
  void (*kernel[3])(const uint8_t *, uint64_t *, const uint64_t *, uint32_t, uint64_t *, int32_t *, uint32_t *,
                    uint64_t, cpk::DecStreams);
  unsigned threads;
  uint32_t lds;
};
const DecForm kDecForms[] = {
    {{cpk::decode_kernel<false>, cpk::decode_kernel<true>, cpk::decode_at_kernel<false>},
     cpk::kDecThreads, cpk::kDecLds},
    {{cpk::decode2_kernel<false>, cpk::decode2_kernel<true>, cpk::decode2_at_kernel}, cpk::kD2Threads, cpk::kD2Lds},
    {{cpk::decode_kernel<false, true>, cpk::decode_kernel<true, true>, cpk::decode_at_kernel<true>},
     cpk::kDecThreads, cpk::kDecLds}};

// one launch of a decoder (grid: as many workgroups per CU as its LDS allows,
// at most 8; never more than the work needs)
void dec_launch(cpk_ctx ctx, DecShape shape, unsigned want, const uint8_t *packed, uint64_t *in_off,
                const uint64_t *swo, uint32_t n, uint64_t *out, int32_t *status, uint64_t avail,
                cpk::DecStreams sd, hipStream_t s, DecKind which = kDecCtx) {
  if (which == kDecCtx) which = dec_ctx_kind(ctx);
  const DecForm &f = kDecForms[which - kDecMap];
  unsigned grid = min(8u, 160u * 1024u / f.lds) * (unsigned)ctx->cus;
  if (grid > want) grid = want;
  if (grid == 0) grid = 1;
  hipLaunchKernelGGL(f.kernel[shape], dim3(grid), dim3(f.threads), f.lds, s, packed, in_off, swo, n, out, status,
                     ctx->tickets + cpk::kTkDec, avail, sd);
}

// The forms a batch call enqueues.  By density (no CPK_DECODER) a gate kernel
// writes dec_skip's three words and launch(kind, its word) runs for all three,
// the ones not chosen return at once; a forced decoder alone, no skip word.
bool dec_gated(cpk_ctx ctx) { return ctx->decoder == 3; }
uint32_t *dec_skip(cpk_ctx ctx) { return ctx->tickets + cpk::kTkGate + cpk::kGateDecSkip; }
template <class F>
void dec_each_form(cpk_ctx ctx, F launch) {
  if (!dec_gated(ctx)) return launch(dec_ctx_kind(ctx), (const uint32_t *)nullptr);
  for (int k = kDecMap; k <= kDecDense; ++k) launch((DecKind)k, (const uint32_t *)dec_skip(ctx) + (k - kDecMap));
}
}  // namespace
extern "C" {

int cpk_decode_batch(cpk_ctx ctx, const void *d_packed, const uint64_t *d_in_off, const uint64_t *d_swo, uint32_t n,
                     void *d_out, int32_t *d_status, void *stream) {
  return decode_batch_impl(ctx, d_packed, d_in_off, d_swo, n, d_out, d_status, stream, may_probe(ctx, n, stream));
}

static int decode_batch_impl(cpk_ctx ctx, const void *d_packed, const uint64_t *d_in_off, const uint64_t *d_swo,
                             uint32_t n, void *d_out, int32_t *d_status, void *stream, bool probe) {
  if (!ctx || (n && (!d_in_off || !d_swo || !d_status))) return CPK_EINVAL;
  if (((uintptr_t)d_packed & 15) || ((uintptr_t)d_out & 7)) return CPK_EINVAL;
  if (n == 0) return CPK_OK;
  DeviceGuard g(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  if (dec_tickets_reset(ctx, s) != hipSuccess) return CPK_EDEVICE;
  // persistent: blocks of 4 independent waves, as many per CU as the LDS holds
  uint64_t *in_off = const_cast<uint64_t *>(d_in_off);
  // by density, decided on the device (a forced decoder: no gate, no probe)
  const bool gate = dec_gated(ctx);
  if (gate)
    hipLaunchKernelGGL(cpk::dec_gate_kernel, dim3(1), dim3(64), 0, s, (const uint64_t *)d_in_off, d_swo, n,
                       dec_skip(ctx));
  if (gate && probe && n <= 32) {
    // A few pieces: read their extent back (one sync).  With >= 8 MiB of
    // words each on average the batch decoders would give a piece one wave
    // (one 64 MiB piece: ~100 ms), so decode them as one stream, 256-byte
    // blocks in parallel, and let the batch decoders skip when every piece
    // ended exactly at its packed range's end (dec_stream_check_kernel);
    // otherwise they run after it and report the batch form's statuses.
    // (through pinned memory: four copies into pageable memory cost ~75 us
    // per call, ADVICE r5, profiles/r6b_small_decode_launch_overhead.txt)
    uint64_t e[4];
    int rc0 = read_words(ctx, s, {d_in_off, d_in_off + n, d_swo, d_swo + n}, e);
    if (rc0) return rc0;
    if (e[3] - e[2] >= ((uint64_t)n << 20) && (e[0] & 15) == 0 && e[1] >= e[0]) {
      if (int rc = reserve_fixed(ctx->fl_buf, 33 * 8)) return rc;
      int rc = cpk_decode_stream(ctx, (const uint8_t *)d_packed + e[0], e[1] - e[0], d_swo, n, d_out, ctx->fl_buf.p,
                                 d_status, s);
      if (rc) return rc;
      hipLaunchKernelGGL(cpk::dec_stream_check_kernel, dim3(1), dim3(64), 0, s, (const uint64_t *)ctx->fl_buf.p,
                         (const uint64_t *)d_in_off, (const int32_t *)d_status, n, dec_skip(ctx));
      if (dec_tickets_reset(ctx, s) != hipSuccess) return CPK_EDEVICE;
    }
  }
  dec_each_form(ctx, [&](DecKind k, const uint32_t *sk) {
    dec_launch(ctx, kDecBatch, (n + 3) / 4, (const uint8_t *)d_packed, in_off, d_swo, n, (uint64_t *)d_out, d_status, 0,
               cpk::DecStreams::batch(sk), s, k);
  });
  return hip_ok(hipGetLastError());
}

namespace {
// streams of at least this many bytes (after the bound below) are cut into
// blocks and decoded in parallel (stream_split.hip); shorter ones by one
// workgroup (decode_mw.hip; one wave under kRmMwMin).  Device-resident
// (tools/stream_bench.py, config-2 data, one piece): 0.32 MiB packed 0.17 ms
// by the workgroup against 0.23 ms by the block path, 0.65 MiB 0.31 / 0.23
constexpr uint64_t kSsMin = 384 * 1024;
constexpr uint64_t kRmSsMin = 64 * 1024;  // cpk_read_message
// cpk_read_message_host: streams under kRmMwMax bytes in one launch (pinned
// memory, no DMA), by one wave (rm_small_kernel) under kRmMwMin, else by a
// whole workgroup (rm_mw_kernel).  Measured (threshold_probe, config-2-like
// messages): one wave 36.7 / mw 42.9 us at 3.9 KB packed, 51.2 / 45.7 at
// 7.8 KB; mw 54 us at 64 KiB of words (one wave 151), 116 at 256 KiB (the
// parallel block path 206)
constexpr uint64_t kRmMwMin = 6 * 1024;
constexpr uint64_t kRmMwMax = 512 * 1024;
// From host memory the workgroup reads the packed bytes straight from pinned
// memory (PCIe round trips per window) and the block path stages them by
// DMA: the block path is ahead from 128 KiB there (passByBytes replay, 512
// KiB messages: 806 us per iteration against 940 at 256 KiB and 1,190 at
// 512 KiB, profiles/r6c_pass_by_bytes_mw*.txt)
constexpr uint64_t kRmMwMaxHost = 128 * 1024;
// the host path's packed bytes on the device: the largest one-launch stream and its read slack
constexpr uint64_t kRmCopyBytes = kRmMwMax + 128;
int rm_copy_reserve(cpk_ctx ctx) { return reserve_fixed(ctx->rm_copy, kRmCopyBytes); }
uint64_t rm_mw_max(cpk_ctx ctx, bool host) {
  const uint64_t d = host ? kRmMwMaxHost : kRmMwMax;
  return ctx->rm_mw_max && ctx->rm_mw_max < kRmMwMax ? ctx->rm_mw_max : d;
}

// the bytes a stream of `words` words may take: 10 per word at most
uint64_t ss_reach(uint64_t avail, uint64_t words) {
  const uint64_t b = words > (~0ull - 16) / 10 ? ~0ull : 10 * words + 16;
  return avail < b ? avail : b;
}

// the block map's scratch for nb blocks, in the context (grown on demand)
int ss_bufs(cpk_ctx ctx, uint64_t nb, cpk::SsBufs &B) {
  using namespace cpk;
  const uint64_t ng = (nb + kSsGroup - 1) / kSsGroup;
  return carve_reserve(ctx->ss_buf, 0, [&](Carve &c) {
    B.X = c.take(nb);
    B.W = c.take(nb);
    B.C1 = c.take(nb);
    B.L1 = c.take(nb);
    B.WL1 = c.take(nb);
    B.C2 = c.take(kSsCand * nb);
    B.L2 = c.take(kSsCand * nb);
    B.WL2 = c.take(kSsCand * nb);
    B.N2 = c.take32(nb);
    B.GE = c.take(kSsVar * ng);
    B.GX = c.take(kSsVar * ng);
    B.GW = c.take(kSsVar * ng);
    B.VE = c.take((kSsVar + 1) * nb);
    B.VW = c.take32((kSsVar + 1) * nb);
    B.GC = c.take32(ng);
    B.GB = c.take(ng);
    B.E = c.take(nb + 1);
    B.WO = c.take(nb + 1);
    B.sin = c.take(nb + 1);
    B.sswo = c.take(nb + 1);
    B.sst = (int32_t *)c.take32(nb);
    B.flag = c.take32(4);
    B.lim = c.take(2);
  });
}

// parallel stream decode over at most `reach` bytes; enqueues the one-wave
// decoder after it, which runs only if the parallel path met anything
// irregular (it then decodes the whole stream, errors included)
int ss_decode(cpk_ctx ctx, const uint8_t *pk, uint64_t avail, uint64_t reach, const uint64_t *swo, uint32_t n,
              uint64_t *out, uint64_t *in_off, int32_t *status, hipStream_t s) {
  using namespace cpk;
  const uint64_t nb = (reach + kSsBlock - 1) / kSsBlock;
  SsBufs B;
  if (int rc = ss_bufs(ctx, nb, B)) return rc;
  if (int rc = ss_map_launch(ctx, pk, reach, swo, n, nb, B, s)) return rc;
  const unsigned tb = 256;
  const uint64_t nsub = (nb + kSsSub - 1) / kSsSub;
  hipLaunchKernelGGL(ss_bound_kernel, dim3((n + 1 + 63) / 64), dim3(64), 0, s, pk, swo, n, nb, in_off, B);
  hipLaunchKernelGGL(ss_sub_kernel, dim3((unsigned)((nsub + 1 + tb - 1) / tb)), dim3(tb), 0, s, swo, n, nb,
                     (const uint64_t *)in_off, B);
  dec_launch(ctx, kDecBatch, (unsigned)((nsub + 3) / 4), pk, B.sin, B.sswo, (uint32_t)nsub, out, B.sst, 0,
             DecStreams::batch(), s);
  hipLaunchKernelGGL(ss_check_kernel, dim3((unsigned)((nsub + tb - 1) / tb)), dim3(tb), 0, s, nsub, B);
  hipLaunchKernelGGL(ss_final_kernel, dim3((n + tb - 1) / tb), dim3(tb), 0, s, n, status, ctx->tickets + kTkDec, B,
                     getenv("CPK_STREAM_NO_FALLBACK") ? 1 : 0);
  // the one-wave decoder: no ticket unless the parallel path gave up
  dec_launch(ctx, kDecStream, 1, pk, in_off, swo, n, out, status, avail, DecStreams::one(in_off + n), s);
  return hip_ok(hipGetLastError());
}
}  // namespace

int cpk_decode_stream(cpk_ctx ctx, const void *d_packed, uint64_t avail,
                      const uint64_t *d_swo, uint32_t n, void *d_out, uint64_t *d_in_off,
                      int32_t *d_status, void *stream) {
  if (!ctx || (n && (!d_in_off || !d_swo || !d_status))) return CPK_EINVAL;
  if (((uintptr_t)d_packed & 15) || ((uintptr_t)d_out & 7)) return CPK_EINVAL;
  if (n == 0) return CPK_OK;
  DeviceGuard g(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  if (avail >= kSsMin && !getenv("CPK_STREAM_ONE_WAVE")) {
    // the stream's word count bounds the bytes worth cutting into blocks
    // (the rest of `avail` may be later messages): read it back
    uint64_t ends[2];
    int rc = read_words(ctx, s, {d_swo, d_swo + n}, ends);
    if (rc) return rc;
    const uint64_t reach = ss_reach(avail, ends[1] - ends[0]);
    if (reach >= kSsMin)
      return ss_decode(ctx, (const uint8_t *)d_packed, avail, reach, d_swo, n, (uint64_t *)d_out, d_in_off,
                       d_status, s);
  }
  if (avail >= kRmMwMin && !getenv("CPK_STREAM_ONE_WAVE")) {
    // a mid-size stream: one workgroup, its 16 waves sharing each piece's windows
    hipLaunchKernelGGL(cpk::stream_mw_kernel, dim3(1), dim3(cpk::kMwThreads), cpk::kMwLds, s,
                       (const uint8_t *)d_packed, avail, d_swo, n, (uint64_t *)d_out, d_in_off, d_status);
    return hip_ok(hipGetLastError());
  }
  if (dec_tickets_reset(ctx, s) != hipSuccess)
    return CPK_EDEVICE;
  // one stream: one wave works, the others find no ticket
  dec_launch(ctx, kDecStream, 1, (const uint8_t *)d_packed, d_in_off, d_swo, n, (uint64_t *)d_out, d_status, avail,
             cpk::DecStreams::one(d_in_off + n), s);
  return hip_ok(hipGetLastError());
}


// A whole stream of packed messages (stream_split.hip, ms_*): the block map
// over every byte, the blocks decoded into d_out, the frame chain, every
// piece boundary checked, the result row read back (the one sync; a second
// only when the chain made more entries than the context had room for).
int cpk_decode_message_stream(cpk_ctx ctx, const void *d_packed, uint64_t avail, uint64_t traversal_limit_words,
                              void *d_out, uint64_t out_cap_words, uint64_t *d_msg_off, uint64_t *d_msg_seg_off,
                              uint32_t msg_cap, uint64_t *d_seg_begin, uint64_t *d_seg_words, uint32_t seg_cap,
                              uint64_t *h_info, void *stream) {
  using namespace cpk;
  if (!ctx || !h_info || (avail && !d_packed) || (out_cap_words && !d_out)) return CPK_EINVAL;
  if (((uintptr_t)d_packed & 15) || ((uintptr_t)d_out & 7) || ((uintptr_t)d_msg_off & 7) ||
      ((uintptr_t)d_msg_seg_off & 7) || ((uintptr_t)d_seg_begin & 7) || ((uintptr_t)d_seg_words & 7))
    return CPK_EINVAL;
  if (seg_cap && (!d_seg_begin || !d_seg_words)) return CPK_EINVAL;
  if (msg_cap && (!d_msg_off || !d_msg_seg_off)) return CPK_EINVAL;
  for (int i = 0; i < CPK_MS_INFO_WORDS; ++i) h_info[i] = 0;
  DeviceGuard g(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  if (avail == 0) {
    if ((d_msg_off && fill_async(d_msg_off, 0, 8, s) != hipSuccess) ||
        (d_msg_seg_off && fill_async(d_msg_seg_off, 0, 8, s) != hipSuccess))
      return CPK_EDEVICE;
    return CPK_OK;
  }
  // (entries the arrays hold: msg_cap + 1 and seg_cap; none without an array)
  const int64_t msg_lim = d_msg_off && d_msg_seg_off ? (int64_t)msg_cap : -1;
  const int64_t seg_lim = d_seg_begin && d_seg_words ? (int64_t)seg_cap : 0;
  const uint64_t nb = (avail + kSsBlock - 1) / kSsBlock;
  SsBufs B;
  if (int rc = ss_bufs(ctx, nb, B)) return rc;
  // the chain's entries: a message per 64 packed bytes to begin with
  auto ms_bufs = [&](uint64_t entries, MsBufs &M) -> int {
    // ctl [8] | result row [8] | X, S, P [cap each] | statuses [cap x i32]
    // (not a Carve layout: this buffer's capacity counts chain entries, its
    // bytes follow from the capacity reserve() settles on, and the kernels
    // are told that capacity -- a layout counted before the reservation
    // would need the count run a second time inside the bytes callback)
    if (int rc = reserve(ctx->ms_buf, entries, 0, [](uint64_t cap) { return (16 + 3 * cap + (cap + 1) / 2) * 8; }))
      return rc;
    M.mcap = ctx->ms_buf.cap;
    M.ctl = ctx->ms_buf.p;
    M.res = M.ctl + 8;
    M.X = M.res + 8;
    M.S = M.X + M.mcap;
    M.P = M.S + M.mcap;
    M.ST = (int32_t *)(M.P + M.mcap);
    return CPK_OK;
  };
  MsBufs M;
  if (int rc = ms_bufs(avail / 64 + 1024, M)) return rc;
  const uint8_t *pk = (const uint8_t *)d_packed;
  const uint64_t *out = (const uint64_t *)d_out;
  if (int rc = ss_map_launch(ctx, pk, avail, nullptr, 0, nb, B, s)) return rc;
  const unsigned tb = 256;
  const uint64_t nsub = (nb + kSsSub - 1) / kSsSub;
  hipLaunchKernelGGL(ms_end_kernel, dim3(1), dim3(64), 0, s, pk, nb, out_cap_words, B, M);
  hipLaunchKernelGGL(ms_sub_kernel, dim3((unsigned)((nsub + 1 + tb - 1) / tb)), dim3(tb), 0, s, nb, B, M);
  dec_launch(ctx, kDecBatch, (unsigned)((nsub + 3) / 4), pk, B.sin, B.sswo, (uint32_t)nsub, (uint64_t *)d_out, B.sst, 0,
             DecStreams::batch(), s);
  hipLaunchKernelGGL(ss_check_kernel, dim3((unsigned)((nsub + tb - 1) / tb)), dim3(tb), 0, s, nsub, B);
  uint64_t r[8];
  for (int attempt = 0;; ++attempt) {
    const unsigned waves = (unsigned)((M.mcap + 3) / 4), bgrid = waves < 8u * ctx->cus ? waves : 8u * ctx->cus;
    hipLaunchKernelGGL(ms_chain_kernel, dim3(1), dim3(64), 0, s, out, nb, B, M, traversal_limit_words,
                       d_msg_seg_off, msg_lim, d_seg_begin, d_seg_words, seg_lim);
    hipLaunchKernelGGL(ms_bound_kernel, dim3(bgrid), dim3(256), 0, s, pk, out, nb, B, M, traversal_limit_words,
                       d_msg_off, msg_lim);
    hipLaunchKernelGGL(ms_final_kernel, dim3(1), dim3(64), 0, s, nb, B, M);
    if (hipGetLastError() != hipSuccess) return CPK_EDEVICE;
    if (int rc = read_words(ctx, s, {M.res, M.res + 1, M.res + 2, M.res + 3, M.res + 4, M.res + 5, M.res + 6,
                                    M.res + 7}, r))
      return rc;
    if (!(r[6] & kMsShort) || attempt) break;
    // more messages than entries: the chain and the checks again with room
    // for all (the map and the words stay as they are)
    if (int rc = ms_bufs(r[5], M)) return rc;
    hipLaunchKernelGGL(ms_rearm_kernel, dim3(1), dim3(64), 0, s, M);
  }
  h_info[2] = r[7];
  if (r[6] & kMsNoRoom) return CPK_ENOMEM;
  if (r[6] & kMsShort) return CPK_EDEVICE;
  if (r[6]) {
    // the batch decoder rejected a block of the map (no such stream is known)
    h_info[2] = 0;
    h_info[4] = (uint64_t)(int64_t)CPK_EUNSUPPORTED;
    return CPK_EUNSUPPORTED;
  }
  h_info[0] = r[0];
  h_info[1] = r[1];
  if ((int64_t)r[0] > msg_lim || (int64_t)r[1] > seg_lim) return CPK_ENOMEM;
  h_info[2] = r[2];
  h_info[3] = r[3];
  h_info[4] = r[4];
  return CPK_OK;
}

// ---- unpacked sizes without decoding (decode_size.hip) ---------------------
// A wave per piece sums its windows' words into the context's workspace, the
// size scan turns them into d_seg_word_off.  A few large pieces (n <= 32)
// would each keep one wave busy for the whole call: where the host knows
// their offsets (h_off, the host form) or may read them back (probe), a large
// piece that starts on a 16-byte line is sized by the block map over its
// bytes alone (ss_map_launch, us_end_kernel); what that cannot settle -- an
// irregular map, a piece ending inside a record -- stays marked in todo and
// the wave form sizes it after all.
// One piece of config-2 data by both forms (tools/bench_unpacked_size.py,
// profiles/unpacked_size_bench.log; DESIGN.md section 4 has the table): one
// wave walks 1 MiB in 1.7 ms, the map's launches take 0.12 ms up to 512 KiB
// and 0.75 ms at 256 MiB -- level at 64 KiB.  The maps of several pieces run
// one after the other while their waves would run side by side, so a piece
// of a batch of n takes the map from n * kUsBlockMin bytes.
constexpr uint64_t kUsBlockMin = 64 * 1024;
// The wave form: persistent workgroups of 4 independent waves, kUsWpe per CU.
// end: the ranges are beg[i] .. end[i] (us_wave_at_kernel); null: beg holds n + 1 offsets.
static void us_wave_launch(cpk_ctx ctx, const uint8_t *pk, const uint64_t *beg, const uint64_t *end, uint32_t n,
                           uint64_t *words, int32_t *status, const uint32_t *todo, hipStream_t s) {
  using namespace cpk;
  const unsigned want = (n + 3) / 4, full = (unsigned)(kUsWpe * ctx->cus);
  const dim3 grid(want < full ? want : full), block(kUsThreads);
  uint32_t *tk = ctx->tickets + kTkDec;
  if (end) hipLaunchKernelGGL(us_wave_at_kernel, grid, block, kUsLds, s, pk, beg, end, n, words, status, tk, todo);
  else hipLaunchKernelGGL(us_wave_kernel, grid, block, kUsLds, s, pk, beg, n, words, status, tk, todo);
}
static int unpacked_size_impl(cpk_ctx ctx, const void *d_packed, const uint64_t *d_in_off, uint32_t n,
                              uint64_t *d_swo, int32_t *d_status, void *stream, bool probe, const uint64_t *h_off) {
  using namespace cpk;
  if (!ctx || !d_swo || (n && (!d_in_off || !d_status))) return CPK_EINVAL;
  if (((uintptr_t)d_packed & 15) || ((uintptr_t)d_in_off & 7) || ((uintptr_t)d_swo & 7) || ((uintptr_t)d_status & 3))
    return CPK_EINVAL;
  DeviceGuard g(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) return hip_ok(fill_async(d_swo, 0, 8, s));
  // words [n] | the scan's block sums | todo [n] (u32)
  uint64_t *words, *bsum;
  uint32_t *todo;
  if (int rc = carve_reserve(ctx->status, 1024, [&](Carve &c) {
        words = c.take(n);
        bsum = c.take(scan_blocks(n) + 1);
        todo = c.take32(n);
      }))
    return rc;
  const uint8_t *pk = (const uint8_t *)d_packed;
  bool mapped = false;
  if (n <= 32 && ctx->usize_form != 2 && (h_off || probe)) {
    uint64_t off[33];
    bool large = ctx->usize_form == 1;
    if (h_off) {
      memcpy(off, h_off, (n + 1) * 8ull);
    } else {
      uint64_t e[2];
      if (int rc = read_words(ctx, s, {d_in_off, d_in_off + n}, e)) return rc;
      off[0] = e[0];
      off[n] = e[1];
      large = large || (e[1] >= e[0] && e[1] - e[0] >= n * kUsBlockMin);
      // the pieces in between (a second small read-back, only on this path)
      if (large && n > 1 &&
          (hipMemcpyAsync(off, d_in_off, (n + 1) * 8ull, hipMemcpyDeviceToHost, s) != hipSuccess ||
           hipStreamSynchronize(s) != hipSuccess))
        return CPK_EDEVICE;
    }
    auto takes = [&](uint32_t i) {
      const uint64_t len = off[i + 1] - off[i];
      return off[i + 1] > off[i] && (off[i] & 15) == 0 && (ctx->usize_form == 1 || len >= n * kUsBlockMin);
    };
    uint64_t nbmax = 0;
    for (uint32_t i = 0; (large || h_off) && i < n; ++i)
      if (takes(i)) nbmax = max(nbmax, (off[i + 1] - off[i] + kSsBlock - 1) / kSsBlock);
    if (nbmax) {
      SsBufs B;
      if (int rc = ss_bufs(ctx, nbmax, B)) return rc;
      if (fill_async(todo, 0xff, (uint64_t)n * 4, s) != hipSuccess) return CPK_EDEVICE;
      for (uint32_t i = 0; i < n; ++i) {
        if (!takes(i)) continue;
        const uint64_t len = off[i + 1] - off[i], nb = (len + kSsBlock - 1) / kSsBlock;
        if (int rc = ss_map_launch(ctx, pk + off[i], len, nullptr, 0, nb, B, s)) return rc;
        hipLaunchKernelGGL(us_end_kernel, dim3(1), dim3(64), 0, s, pk + off[i], nb, B, words + i, d_status + i,
                           todo + i);
      }
      mapped = true;
    }
  }
  if (dec_tickets_reset(ctx, s) != hipSuccess) return CPK_EDEVICE;
  us_wave_launch(ctx, pk, d_in_off, nullptr, n, words, d_status, mapped ? todo : nullptr, s);
  scan_launch(words, n, bsum, d_swo, s);
  return hip_ok(hipGetLastError());
}

int cpk_unpacked_size_batch(cpk_ctx ctx, const void *d_packed, const uint64_t *d_in_off, uint32_t n,
                            uint64_t *d_seg_word_off, int32_t *d_status, void *stream) {
  // (a batch of <= 32 pieces may read its extent back, as cpk_decode_batch does)
  return unpacked_size_impl(ctx, d_packed, d_in_off, n, d_seg_word_off, d_status, stream,
                            n > 0 && may_probe(ctx, n, stream), nullptr);
}

// ---- decode from caller-given ranges (decode_at.hip) -------------------------
// The ranges checked and the batch's packed bytes summed (dat_prep_kernel), the
// decoder chosen on the device from that sum (dat_gate_kernel; a forced
// decoder alone), the groups' statuses and consumed bytes (dat_final_kernel).
// No groups given: the batch forms on a range per piece; groups: the stream
// forms, a wave per group, the groups with the most packed bytes first.
int cpk_decode_batch_at(cpk_ctx ctx, const void *d_packed, uint64_t in_cap, const uint64_t *d_src_off,
                        const uint64_t *d_src_len, const uint64_t *d_grp_piece_off, uint32_t ng,
                        const uint64_t *d_seg_word_off, uint32_t n, void *d_out, int32_t *d_status,
                        int32_t *d_grp_status, uint64_t *d_grp_used, void *stream) {
  using namespace cpk;
  if (!ctx || (n && (!d_seg_word_off || !d_status))) return CPK_EINVAL;
  if (ng && (!d_src_off || !d_src_len || !d_grp_status || !d_grp_used)) return CPK_EINVAL;
  if (d_grp_piece_off ? (ng == 0 && n != 0) : ng != n) return CPK_EINVAL;
  if (((uintptr_t)d_packed & 15) || ((uintptr_t)d_out & 7) || ((uintptr_t)d_status & 3) ||
      ((uintptr_t)d_grp_status & 3))
    return CPK_EINVAL;
  for (const void *q : {(const void *)d_src_off, (const void *)d_src_len, (const void *)d_grp_piece_off,
                        (const void *)d_seg_word_off, (const void *)d_grp_used})
    if ((uintptr_t)q & 7) return CPK_EINVAL;
  if (ng == 0) return CPK_OK;
  DeviceGuard g(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  const bool grouped = d_grp_piece_off != nullptr;
  // begin | end | pieces' end [ng]; the packed sum; with groups their lengths
  // and order, and the pieces' starts the stream forms write
  uint64_t *gbeg, *gend, *gout, *psum, *glen = nullptr, *pin = nullptr;
  uint32_t *ord = nullptr, *ohist = nullptr;
  if (int rc = carve_reserve(ctx->status, 1024, [&](Carve &c) {
        gbeg = c.take(3ull * ng);  // (no groups: begin | end | out per piece, interleaved)
        gend = gbeg ? gbeg + (grouped ? ng : 1) : nullptr;
        gout = gbeg ? gbeg + (grouped ? 2ull * ng : 2) : nullptr;
        psum = c.take(1);
        if (grouped) {
          glen = c.take(ng);
          pin = c.take(n);
          ord = c.take32(ng);
          ohist = c.take32(kOrdClasses);
        }
      }))
    return rc;
  if (fill_async(psum, 0, 8, s) != hipSuccess || dec_tickets_reset(ctx, s) != hipSuccess) return CPK_EDEVICE;
  DatArgs A = {d_src_off, d_src_len, d_grp_piece_off, d_seg_word_off, n,          ng,
               in_cap,    gbeg,      gend,            gout,           grouped ? 1u : 3u, d_grp_status};
  const unsigned gg = (ng + kDatThreads - 1) / kDatThreads;
  hipLaunchKernelGGL(dat_prep_kernel, dim3(gg), dim3(kDatThreads), 0, s, A, (unsigned long long *)psum, glen,
                     (uint64_t *)nullptr, (uint32_t *)nullptr);
  if (n) {
    const uint8_t *pk = (const uint8_t *)d_packed;
    if (dec_gated(ctx))
      hipLaunchKernelGGL(dat_gate_kernel, dim3(1), dim3(64), 0, s, (const unsigned long long *)psum, d_seg_word_off,
                         n, dec_skip(ctx));
    if (grouped) ord_launch(glen, ng, ohist, ord, s);
    // groups: the stream forms; none: the batch forms on a range per piece
    dec_each_form(ctx, [&](DecKind k, const uint32_t *sk) {
      if (grouped)
        dec_launch(ctx, kDecStream, (ng + 3) / 4, pk, pin, d_seg_word_off, n, (uint64_t *)d_out, d_status, 0,
                   DecStreams{gbeg, gend, d_grp_piece_off, ng, gout, sk, ord}, s, k);
      else
        dec_launch(ctx, kDecAt, (n + 3) / 4, pk, gbeg, d_seg_word_off, n, (uint64_t *)d_out, d_status, (uint64_t)0,
                   DecStreams::batch(sk), s, k);
    });
  }
  hipLaunchKernelGGL(dat_final_kernel, dim3(gg), dim3(kDatThreads), 0, s, A, d_status, d_grp_used);
  return hip_ok(hipGetLastError());
}

// cpk_unpacked_size_batch over n ranges: the wave-per-piece form alone (no
// read-back, no block map), refused ranges sized 0 by dat_prep_kernel.
int cpk_unpacked_size_batch_at(cpk_ctx ctx, const void *d_packed, uint64_t in_cap, const uint64_t *d_src_off,
                               const uint64_t *d_src_len, uint32_t n, uint64_t *d_seg_word_off, int32_t *d_status,
                               void *stream) {
  using namespace cpk;
  if (!ctx || !d_seg_word_off || (n && (!d_src_off || !d_src_len || !d_status))) return CPK_EINVAL;
  if (((uintptr_t)d_packed & 15) || ((uintptr_t)d_src_off & 7) || ((uintptr_t)d_src_len & 7) ||
      ((uintptr_t)d_seg_word_off & 7) || ((uintptr_t)d_status & 3))
    return CPK_EINVAL;
  DeviceGuard g(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) return hip_ok(fill_async(d_seg_word_off, 0, 8, s));
  // words [n] | the scan's block sums | begin | end [n] | todo [n] (u32)
  uint64_t *words, *bsum, *gbeg, *gend;
  uint32_t *todo;
  if (int rc = carve_reserve(ctx->status, 1024, [&](Carve &c) {
        words = c.take(n);
        bsum = c.take(scan_blocks(n) + 1);
        gbeg = c.take(n);
        gend = c.take(n);
        todo = c.take32(n);
      }))
    return rc;
  if (dec_tickets_reset(ctx, s) != hipSuccess) return CPK_EDEVICE;
  DatArgs A = {d_src_off, d_src_len, nullptr, nullptr, n, n, in_cap, gbeg, gend, nullptr, 1u, d_status};
  hipLaunchKernelGGL(dat_prep_kernel, dim3((n + kDatThreads - 1) / kDatThreads), dim3(kDatThreads), 0, s, A,
                     (unsigned long long *)nullptr, (uint64_t *)nullptr, words, todo);
  us_wave_launch(ctx, (const uint8_t *)d_packed, gbeg, gend, n, words, d_status, todo, s);
  scan_launch(words, n, bsum, d_seg_word_off, s);
  return hip_ok(hipGetLastError());
}

// ---- messages from caller-given ranges (decode_msg_at.hip) --------------------
// The tables read from the ranges (mat_table_kernel), the accepted messages'
// words and segment counts scanned, the capacity verdict and the decoders'
// piece ranges made on the device (mat_fit_kernel, mat_place_kernel), the
// decoder chosen there too (dat_gate_kernel over the fitting messages; a
// forced decoder alone), the stream forms a wave per message, the statuses and
// consumed bytes (mat_final_kernel).  Nothing is read back: the host decides
// on its own arguments only.
int cpk_decode_messages_at(cpk_ctx ctx, const void *d_packed, uint64_t in_cap, const uint64_t *d_src_off,
                           const uint64_t *d_src_len, uint32_t nm, uint64_t traversal_limit_words, void *d_out,
                           uint64_t out_cap_words, uint64_t *d_seg_word_off, uint64_t *d_seg_in_off,
                           int32_t *d_seg_status, uint32_t seg_cap, uint64_t *d_msg_seg_off, int32_t *d_msg_status,
                           uint64_t *d_msg_used, uint64_t *d_totals, void *stream) {
  using namespace cpk;
  if (!ctx || !d_msg_seg_off || !d_totals) return CPK_EINVAL;
  if (nm && (!d_src_off || !d_src_len || !d_msg_status || !d_msg_used)) return CPK_EINVAL;
  if ((seg_cap && (!d_seg_word_off || !d_seg_in_off || !d_seg_status)) || (out_cap_words && !d_out))
    return CPK_EINVAL;
  if (((uintptr_t)d_packed & 15) || ((uintptr_t)d_out & 7) || ((uintptr_t)d_seg_status & 3) ||
      ((uintptr_t)d_msg_status & 3))
    return CPK_EINVAL;
  for (const void *q : {(const void *)d_src_off, (const void *)d_src_len, (const void *)d_seg_word_off,
                        (const void *)d_seg_in_off, (const void *)d_msg_seg_off, (const void *)d_msg_used,
                        (const void *)d_totals})
    if ((uintptr_t)q & 7) return CPK_EINVAL;
  DeviceGuard g(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  if (nm == 0) {
    if (fill_async(d_msg_seg_off, 0, 8, s) != hipSuccess) return CPK_EDEVICE;
    return hip_ok(fill_async(d_totals, 0, 8 * CPK_MAT_TOTALS, s));
  }
  // the messages' words | first segment bytes | range ends | streams' ends [nm];
  // the words' scan | the decoders' piece ranges [nm + 1]; the two scans' block
  // sums; the fit pass's words; the streams largest first
  uint64_t *mwords, *mbeg, *mend, *mout, *mwoff, *spc, *bs0, *bs1, *fit;
  uint32_t *ord, *ohist;
  if (int rc = carve_reserve(ctx->status, 1024, [&](Carve &c) {
        mwords = c.take(nm);
        mbeg = c.take(nm);
        mend = c.take(nm);
        mout = c.take(nm);
        mwoff = c.take((uint64_t)nm + 1);
        spc = c.take((uint64_t)nm + 1);
        bs0 = c.take(scan_blocks(nm));
        bs1 = c.take(scan_blocks(nm));
        fit = c.take(kMatWords);
        ord = c.take32(nm);
        ohist = c.take32(kOrdClasses);
      }))
    return rc;
  if (fill_async(fit + kMatNoFit, 0xff, 8, s) != hipSuccess ||
      fill_async(fit + kMatCount, 0, 16, s) != hipSuccess)
    return CPK_EDEVICE;
  const uint8_t *pk = (const uint8_t *)d_packed;
  const unsigned tg = (nm + kMatThreads - 1) / kMatThreads, tg1 = nm / kMatThreads + 1;
  // the segment counts go to d_msg_seg_off[0..nm) and are scanned into it, as
  // cpk_decode_messages scans them
  hipLaunchKernelGGL(mat_table_kernel, dim3(tg), dim3(kMatThreads), 0, s, pk, d_src_off, d_src_len, nm, in_cap,
                     traversal_limit_words, mwords, d_msg_seg_off, mbeg, mend, d_msg_status);
  scan_launch(mwords, nm, bs0, mwoff, s);
  scan_launch(d_msg_seg_off, nm, bs1, d_msg_seg_off, s);
  hipLaunchKernelGGL(mat_fit_kernel, dim3(tg), dim3(kMatThreads), 0, s, nm, (const uint64_t *)mwoff,
                     (const uint64_t *)d_msg_seg_off, d_src_len, (const int32_t *)d_msg_status, out_cap_words,
                     (uint64_t)seg_cap, (unsigned long long *)fit);
  hipLaunchKernelGGL(mat_place_kernel, dim3(tg1), dim3(kMatThreads), 0, s, pk, d_src_off, d_src_len, nm,
                     traversal_limit_words, (const uint64_t *)mwoff, (const uint64_t *)d_msg_seg_off, fit, mbeg, mend,
                     spc, d_msg_status, d_seg_word_off, d_seg_in_off, d_totals);
  // (no room for a segment: no message fits, there is nothing to decode)
  if (seg_cap) {
    if (dec_tickets_reset(ctx, s) != hipSuccess) return CPK_EDEVICE;
    if (dec_gated(ctx))
      hipLaunchKernelGGL(dat_gate_kernel, dim3(1), dim3(64), 0, s, (const unsigned long long *)(fit + kMatBytes),
                         (const uint64_t *)(fit + kMatGate), 1u, dec_skip(ctx));
    ord_launch(mwords, nm, ohist, ord, s);
    dec_each_form(ctx, [&](DecKind k, const uint32_t *sk) {
      dec_launch(ctx, kDecStream, (nm + 3) / 4, pk, d_seg_in_off, d_seg_word_off, seg_cap, (uint64_t *)d_out,
                 d_seg_status, 0, DecStreams{mbeg, mend, spc, nm, mout, sk, ord}, s, k);
    });
  }
  hipLaunchKernelGGL(mat_final_kernel, dim3(tg), dim3(kMatThreads), 0, s, nm, d_src_off, d_src_len,
                     (const uint64_t *)spc, (const uint64_t *)mout, (const int32_t *)d_seg_status, d_msg_status,
                     d_msg_used);
  return hip_ok(hipGetLastError());
}

// A whole stream of unpacked messages packed (encode_ms.hip): the frame
// chain over the words, its result row read back (the piece count sizes the
// encoders' launches), the pieces through cpk_encode_batch_cap, then the
// packed total and the context's error word read back.
int cpk_encode_message_stream(cpk_ctx ctx, const void *d_in, uint64_t avail_words, uint64_t traversal_limit_words,
                              void *d_out, uint64_t out_cap, uint64_t *d_out_off, uint32_t piece_cap,
                              uint64_t *d_msg_piece, uint32_t msg_cap, uint64_t *h_info, void *stream) {
  using namespace cpk;
  if (!ctx || !h_info || (avail_words && !d_in) || (out_cap && !d_out)) return CPK_EINVAL;
  if (((uintptr_t)d_in & 7) || ((uintptr_t)d_out & 15) || ((uintptr_t)d_out_off & 7) || ((uintptr_t)d_msg_piece & 7))
    return CPK_EINVAL;
  if ((piece_cap && !d_out_off) || (msg_cap && !d_msg_piece)) return CPK_EINVAL;
  for (int i = 0; i < CPK_EMS_INFO_WORDS; ++i) h_info[i] = 0;
  DeviceGuard g(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  if (avail_words == 0) {
    if ((d_out_off && fill_async(d_out_off, 0, 8, s) != hipSuccess) ||
        (d_msg_piece && fill_async(d_msg_piece, 0, 8, s) != hipSuccess))
      return CPK_EDEVICE;
    return CPK_OK;
  }
  // (the last entry each array holds; none without an array.  A message of
  // `count` segments is 1 + count pieces in at least 1 + count / 2 words:
  // at most two pieces per word)
  const int64_t msg_lim = d_msg_piece ? (int64_t)msg_cap : -1;
  const uint64_t pmax = avail_words > 0x7fffffffull ? 0xffffffffull : 2 * avail_words;
  const int64_t piece_lim = d_out_off ? (int64_t)(piece_cap < pmax ? piece_cap : pmax) : -1;
  const uint64_t offs = (uint64_t)(piece_lim + 1);
  if (int rc = reserve(ctx->ems_buf, offs, 1024, [](uint64_t cap) { return (kEmsRow + cap) * 8; })) return rc;
  uint64_t *row = ctx->ems_buf.p, *poff = ctx->ems_buf.p + kEmsRow;
  const uint64_t *errw = reinterpret_cast<const uint64_t *>(ctx->tickets + kTkErr);  // (the low half)
  hipLaunchKernelGGL(ems_chain_kernel, dim3(1), dim3(64), 0, s, (const uint64_t *)d_in, avail_words,
                     traversal_limit_words, poff, piece_lim, d_msg_piece, msg_lim, row);
  if (hipGetLastError() != hipSuccess) return CPK_EDEVICE;
  uint64_t r[6];
  if (int rc = read_words(ctx, s, {row + kEmsMsgs, row + kEmsPieces, row + kEmsWords, row + kEmsTail,
                                   row + kEmsMax, errw}, r))
    return rc;
  const uint32_t err0 = (uint32_t)r[5];  // (what earlier encodes left for cpk_ctx_take_error)
  h_info[0] = r[0];
  h_info[1] = r[1];
  if ((int64_t)r[0] > msg_lim || (int64_t)r[1] > piece_lim) return CPK_ENOMEM;
  h_info[2] = r[2];
  h_info[4] = r[3];
  h_info[5] = r[4];
  const uint32_t n = (uint32_t)r[1];
  if (n == 0) return hip_ok(fill_async(d_out_off, 0, 8, s));
  // (every piece of a complete message is under 2^28 words and the tables
  // are not empty: the largest piece is a bound the batch call takes)
  if (int rc = cpk_encode_batch_cap(ctx, d_in, poff, n, r[4], d_out, out_cap, d_out_off, stream)) return rc;
  // the packed total: the encoders write the last offset whatever the
  // capacity (the scans; the single pass's look-back); the capacity verdict
  // follows from it, and the error word tells a wait that timed out
  uint64_t e[2];
  if (int rc = read_words(ctx, s, {d_out_off + n, errw}, e)) return rc;
  h_info[3] = e[0];
  const uint32_t err1 = (uint32_t)e[1];
  if ((err1 & ~err0) & (kErrWait | kErrHint)) return CPK_EDEVICE;
  if (e[0] > out_cap) {
    // (reported by the return value: the bit the encoders set for it is
    // taken back unless an earlier call's is still waiting to be taken)
    if (!(err0 & kErrCap) && hipMemsetD32Async((hipDeviceptr_t)(ctx->tickets + kTkErr), (int)(err1 & ~kErrCap), 1, s) !=
                                 hipSuccess)
      return CPK_EDEVICE;
    return CPK_ENOMEM;
  }
  return CPK_OK;
}
}  // extern "C"
static int read_message_impl(cpk_ctx ctx, const void *d_packed, uint64_t avail, uint64_t traversal_limit_words,
                             void *d_out, uint64_t out_cap_words, uint64_t *d_info, void *stream,
                             uint64_t *info_mirror, uint64_t seq = 0, bool *flagged = nullptr);
extern "C" {
int cpk_read_message(cpk_ctx ctx, const void *d_packed, uint64_t avail, uint64_t traversal_limit_words,
                     void *d_out, uint64_t out_cap_words, uint64_t *d_info, void *stream) {
  return read_message_impl(ctx, d_packed, avail, traversal_limit_words, d_out, out_cap_words, d_info, stream,
                           nullptr);
}
}  // extern "C"

// (info_mirror: where rm_final_kernel also copies the info row, e.g. pinned
// host memory read after one sync; d_info null: a device row in rm_buf;
// *flagged set: the one-launch kernel took it and writes seq to
// info_mirror[kRmInfo] when done)
static int read_message_impl(cpk_ctx ctx, const void *d_packed, uint64_t avail, uint64_t traversal_limit_words,
                             void *d_out, uint64_t out_cap_words, uint64_t *d_info, void *stream,
                             uint64_t *info_mirror, uint64_t seq, bool *flagged) {
  if (flagged) *flagged = false;
  using cpk::kRmPieces;
  if (!ctx || (!d_info && !info_mirror) || (avail && !d_packed) || !d_out) return CPK_EINVAL;
  if (((uintptr_t)d_packed & 15) || ((uintptr_t)d_out & 7)) return CPK_EINVAL;
  DeviceGuard g(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  uint64_t *swo, *in_off, *sdesc, *send_out, *npad, *info_row;
  int32_t *pst;
  if (int rc = carve_reserve(ctx->rm_buf, 0, [&](Carve &c) {
        swo = c.take(kRmPieces + 1);
        in_off = c.take(kRmPieces + 1);
        pst = (int32_t *)c.take32(kRmPieces);  // statuses
        sdesc = c.take(4);                     // the stream descriptor
        send_out = c.take(1);                  // the stream's end
        npad = c.take(1);                      // pieces
        c.take(2);                             // (spare)
        info_row = c.take(cpk::kRmInfo);
      }, true))
    return rc;
  if (!d_info) d_info = info_row;
  // the pieces' sizes are on the device only: the stream decoder is sized by
  // the bytes the caller's capacity can reach (10 per word at most)
  const uint64_t reach = ss_reach(avail, out_cap_words + cpk::kRmHead);
  // (a lower bar than cpk_decode_stream's: a message's one-wave decode is
  //  ~0.5 GB/s, the parallel path ~250 us of fixed cost: even at 64 KiB)
  const bool one = getenv("CPK_STREAM_ONE_WAVE") != nullptr;
  if (!one && !dec_v2(ctx) && reach >= kRmMwMin && reach < rm_mw_max(ctx, info_mirror != nullptr)) {
    // (the host path: pinned bytes, copied to the device in the kernel)
    if (info_mirror && rm_copy_reserve(ctx)) return CPK_ENOMEM;
    hipLaunchKernelGGL(cpk::rm_mw_kernel, dim3(1), dim3(cpk::kMwThreads), cpk::kMwLds, s,
                       (const uint8_t *)d_packed, avail, traversal_limit_words, out_cap_words, swo, d_info, sdesc,
                       (uint64_t *)d_out, in_off, pst, send_out, info_mirror,
                       info_mirror ? (uint8_t *)ctx->rm_copy.p : nullptr, seq);
    if (flagged) *flagged = info_mirror != nullptr;
    return hip_ok(hipGetLastError());
  }
  const bool par = reach >= kRmSsMin && !one;
  if (!par && !dec_v2(ctx)) {
    // (the host path's packed bytes are pinned host memory: copied to the
    // device once, in the kernel)
    uint8_t *dcopy = nullptr;
    if (info_mirror && reach + 96 <= kRmCopyBytes) {
      if (rm_copy_reserve(ctx)) return CPK_ENOMEM;
      dcopy = (uint8_t *)ctx->rm_copy.p;
    }
    hipLaunchKernelGGL(cpk::rm_small_kernel, dim3(1), dim3(cpk::kDecThreads), cpk::kDecLds, s,
                       (const uint8_t *)d_packed, avail, traversal_limit_words, out_cap_words, swo, d_info, sdesc,
                       ctx->tickets + cpk::kTkDec, (uint64_t *)d_out, in_off, pst, send_out, info_mirror, dcopy,
                       seq);
    if (flagged) *flagged = info_mirror != nullptr;
    return hip_ok(hipGetLastError());
  }
  hipLaunchKernelGGL(cpk::rm_table_kernel, dim3(1), dim3(64), 0, s, (const uint8_t *)d_packed, avail,
                     traversal_limit_words, out_cap_words, swo, d_info, sdesc,
                     par ? (uint32_t *)nullptr : ctx->tickets + cpk::kTkDec);
  int rc;
  if (par) {
    // every piece, the padding included, gets a status; the last carries the stream's
    rc = ss_decode(ctx, (const uint8_t *)d_packed, avail, reach, swo, kRmPieces, (uint64_t *)d_out, in_off, pst, s);
  } else {
    // one wave over the table's pieces and the segments (the piece count is
    // on the device: a one-stream descriptor), none of the padding; its
    // tickets were zeroed by rm_table_kernel
    dec_launch(ctx, kDecStream, 1, (const uint8_t *)d_packed, in_off, swo, kRmPieces, (uint64_t *)d_out, pst, avail,
               cpk::DecStreams::one_desc(sdesc, send_out), s);
    rc = hip_ok(hipGetLastError());
  }
  if (rc) return rc;
  hipLaunchKernelGGL(cpk::rm_final_kernel, dim3(1), dim3(64), 0, s, par ? (const uint64_t *)(in_off + kRmPieces)
                                                                        : (const uint64_t *)send_out,
                     (const int32_t *)pst, par ? (const uint64_t *)npad : (const uint64_t *)(sdesc + 3), d_info,
                     info_mirror);
  return hip_ok(hipGetLastError());
}
extern "C" {

int cpk_decode_messages(cpk_ctx ctx, const void *d_packed, const uint64_t *d_msg_off, uint32_t nm,
                        uint64_t traversal_limit_words, void *d_out, uint64_t out_cap_words,
                        uint64_t *d_seg_word_off, uint64_t *d_seg_in_off, int32_t *d_seg_status,
                        uint32_t seg_cap, uint64_t *d_msg_seg_off, int32_t *d_msg_status,
                        uint64_t *h_totals, void *stream) {
  if (!ctx || !h_totals || (nm && (!d_msg_off || !d_msg_seg_off || !d_msg_status))) return CPK_EINVAL;
  if (((uintptr_t)d_packed & 15) || ((uintptr_t)d_out & 7)) return CPK_EINVAL;
  h_totals[0] = h_totals[1] = 0;
  DeviceGuard g(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  if (nm == 0) return hip_ok(fill_async(d_msg_seg_off, 0, 8, s));
  uint64_t *mwords, *mbeg, *mwoff, *bs0, *bs1;
  uint32_t *ord, *ohist;
  if (int rc = carve_reserve(ctx->status, 1024, [&](Carve &c) {
        mwords = c.take(nm);  // the messages' words, then their streams' ends
        mbeg = c.take(nm);
        mwoff = c.take((uint64_t)nm + 1);
        bs0 = c.take(scan_blocks(nm));  // the two scans' block sums
        bs1 = c.take(scan_blocks(nm));
        ord = c.take32(nm);  // the streams largest first
        ohist = c.take32(cpk::kOrdClasses);
      }))
    return rc;
  const unsigned tb = 256, tg = (nm + tb - 1) / tb;
  // the segment counts go to d_msg_seg_off[0..nm) and are scanned into it
  // (e4_scan_down: each thread reads its entries before it writes them)
  hipLaunchKernelGGL(cpk::msg_table_kernel, dim3(tg), dim3(tb), 0, s, (const uint8_t *)d_packed,
                     d_msg_off, nm, traversal_limit_words, mwords, d_msg_seg_off, mbeg, d_msg_status);
  scan_launch(mwords, nm, bs0, mwoff, s);
  scan_launch(d_msg_seg_off, nm, bs1, d_msg_seg_off, s);
  uint64_t pk[2] = {0, 0};  // the messages' packed range (the decoder's density choice)
  if (hipGetLastError() != hipSuccess) return CPK_EDEVICE;
  {
    uint64_t w[4];
    const int rcw = read_words(ctx, s, {mwoff + nm, d_msg_seg_off + nm, d_msg_off, d_msg_off + nm}, w);
    if (rcw) return rcw;
    h_totals[0] = w[0];
    h_totals[1] = w[1];
    pk[0] = w[2];
    pk[1] = w[3];
  }
  if (h_totals[0] > out_cap_words || h_totals[1] > seg_cap) return CPK_ENOMEM;
  if (h_totals[1] && (!d_seg_word_off || !d_seg_in_off || !d_seg_status)) return CPK_EINVAL;
  if (!d_seg_word_off) return CPK_OK;  // (no segments: every table failed)
  hipLaunchKernelGGL(cpk::msg_swo_kernel, dim3(tg), dim3(tb), 0, s, (const uint8_t *)d_packed,
                     d_msg_off, nm, traversal_limit_words, (const uint64_t *)mwoff,
                     (const uint64_t *)d_msg_seg_off, (const int32_t *)d_msg_status, d_seg_word_off);
  if (h_totals[1]) {
    if (dec_tickets_reset(ctx, s) != hipSuccess)
      return CPK_EDEVICE;
    // the messages' streams largest first (ord_*: a counting sort by size class)
    ord_launch(mwords, nm, ohist, ord, s);
    // the stream ends overwrite the words array (no longer needed); dense
    // batches (packed bytes >= 80 % of the words') take the block map's
    // dense form, as dec_gate_kernel picks it for cpk_decode_batch (config 3:
    // 48.0 -> 44.4 ms once the stream form's uniform values sat in scalar
    // registers -- with 36 B/lane of spills it had been 49.9,
    // profiles/r5aa_stream_sgpr.txt)
    const bool dense = ctx->decoder == 3 && pk[1] >= pk[0] && 100 * (pk[1] - pk[0]) >= 80 * 8 * h_totals[0];
    dec_launch(ctx, kDecStream, (nm + 3) / 4, (const uint8_t *)d_packed, d_seg_in_off, (const uint64_t *)d_seg_word_off,
               (uint32_t)h_totals[1], (uint64_t *)d_out, d_seg_status, 0,
               cpk::DecStreams::many(mbeg, d_msg_off + 1, d_msg_seg_off, nm, mwords, ord), s,
               dense ? kDecDense : kDecCtx);
    hipLaunchKernelGGL(cpk::msg_final_kernel, dim3(tg), dim3(tb), 0, s, d_msg_off, nm,
                       (const uint64_t *)d_msg_seg_off, (const uint64_t *)mwords,
                       (const int32_t *)d_seg_status, d_msg_status);
  }
  return hip_ok(hipGetLastError());
}

int cpk_decode_stream_host(cpk_ctx ctx, const void *h_packed, uint64_t avail,
                           const uint64_t *h_swo, uint32_t n, void *h_out, uint64_t *h_in_off,
                           int32_t *h_status) {
  if (!ctx || !h_swo || !h_in_off || !h_status) return CPK_EINVAL;
  if (n == 0) {
    h_in_off[0] = 0;
    return CPK_OK;
  }
  for (uint32_t i = 0; i < n; ++i)
    if (h_swo[i + 1] < h_swo[i]) return CPK_EINVAL;
  const uint64_t words = h_swo[n] - h_swo[0];
  if ((!h_packed && avail) || (!h_out && words)) return CPK_EINVAL;
  DeviceGuard g(ctx->device);
  // only the bytes the stream can reach are staged (the rest of `avail` may
  // be later messages), through the context's pinned slot 0 (grow-only: no
  // allocation once it is large enough)
  const uint64_t R = ss_reach(avail, words);
  HostPipe *p = nullptr;
  // meta: swo | in_off | status (int32)
  int rc = pipe_get(ctx, R, words * 8, 2 * (n + 1ull) + n / 2 + 1, &p, 1);
  if (rc) return rc;
  PipeGuard guard{p};
  HostSlot &sl = p->slot[0];
  uint64_t *m = sl.pin_meta, *dm = sl.d_meta;
  for (uint32_t i = 0; i <= n; ++i) m[i] = h_swo[i] - h_swo[0];
  if (hipMemcpyAsync(dm, m, (n + 1) * 8ull, hipMemcpyHostToDevice, p->sk) ||
      stage_in(sl, h_packed, R, 64, p->sk))  // (64: the decoder's read slack)
    return CPK_EDEVICE;
  rc = cpk_decode_stream(ctx, sl.d_in, R, dm, n, sl.d_out, dm + n + 1, (int32_t *)(dm + 2 * (n + 1ull)), p->sk);
  if (rc) return rc;
  if (hipMemcpyAsync(m + n + 1, dm + n + 1, (n + 1) * 8ull + n * 4ull, hipMemcpyDeviceToHost, p->sk) ||
      stage_out(sl, (uint8_t *)h_out + 8 * h_swo[0], sl.d_out, words * 8, p->sk))
    return CPK_EDEVICE;
  guard.done();
  memcpy(h_in_off, m + n + 1, (n + 1) * 8ull);
  memcpy(h_status, m + 2 * (n + 1ull), n * 4ull);
  for (uint32_t i = 0; i < n; ++i)
    if (h_status[i] != CPK_OK) return h_status[i];
  return CPK_OK;
}

// The info row a read left, for the caller: its head (status, bytes consumed,
// segment count, words needed) and, for a message read whole, the segment
// offsets from the first segment's word.  -> the status; w0, words: the
// segments only in the decoder's output (the table's words lead it)
static int rm_info_out(const uint64_t *info, uint64_t *h_info, uint64_t &w0, uint64_t &words) {
  const int st = (int)(int64_t)info[0];
  const uint32_t count = (uint32_t)info[2];
  for (int i = 0; i < 4; ++i) h_info[i] = info[i];
  if (st != CPK_OK) return st;
  w0 = info[4];
  words = info[4 + count] - w0;
  for (uint32_t i = 0; i <= count; ++i) h_info[4 + i] = info[4 + i] - w0;
  return CPK_OK;
}

int cpk_read_message_host(cpk_ctx ctx, const void *h_packed, uint64_t avail, uint64_t traversal_limit_words,
                          void *h_out, uint64_t out_cap_words, uint64_t *h_info) {
  using cpk::kRmInfo;
  if (!ctx || !h_info || (avail && !h_packed) || (out_cap_words && !h_out)) return CPK_EINVAL;
  DeviceGuard g(ctx->device);
  // only the bytes the caller's capacity can reach are staged (the rest of
  // `avail` may be later messages)
  const uint64_t R = ss_reach(avail, out_cap_words + cpk::kRmHead);
  HostPipe *p = nullptr;
  int rc = pipe_get(ctx, R, (out_cap_words + cpk::kRmHead) * 8, kRmInfo + 1, &p, 1);
  if (rc) return rc;
  PipeGuard guard{p};
  HostSlot &sl = p->slot[0];
  uint64_t *info = sl.pin_meta;
  TrClock tc(ctx);
  if (R < rm_mw_max(ctx, true) && !getenv("CPK_NO_SMALL")) {
    // the one-wave range: the kernels read the packed bytes from the pinned
    // slot and write the words and the info row into pinned memory in place
    // -- no DMA either way, one sync
    memcpy(sl.pin_in, h_packed, R);
    memset((uint8_t *)sl.pin_in + R, 0, 64);
    tc.mark(kTrRIn);
    const uint64_t seq = small_arm(ctx, info + kRmInfo);
    bool flagged = false;
    rc = read_message_impl(ctx, sl.pin_in, R, traversal_limit_words, sl.pin_out, out_cap_words, nullptr, p->sk,
                           info, seq, &flagged);
    if (rc) return rc;
    tc.mark(kTrRLaunch);
    if (flagged ? small_wait(ctx, p->sk, info + kRmInfo, seq) : hipStreamSynchronize(p->sk)) return CPK_EDEVICE;
    guard.done();
    tc.mark(kTrRWait);
    uint64_t w0, words;
    if (int st = rm_info_out(info, h_info, w0, words)) return st;
    if (words) memcpy(h_out, (const uint64_t *)sl.pin_out + w0, words * 8);
    tc.mark(kTrROut);
    return CPK_OK;
  }
  // (the bytes chunk by chunk, DMA under the host copy; then the decoder's
  // 64 bytes of read slack)
  if (stage_in(sl, h_packed, R, 64, p->sk)) return CPK_EDEVICE;
  tc.mark(kTrRIn);
  rc = cpk_read_message(ctx, sl.d_in, R, traversal_limit_words, sl.d_out, out_cap_words, sl.d_meta, p->sk);
  if (rc) return rc;
  if (hipMemcpyAsync(info, sl.d_meta, kRmInfo * 8ull, hipMemcpyDeviceToHost, p->sk)) return CPK_EDEVICE;
  tc.mark(kTrRLaunch);
  if (hipStreamSynchronize(p->sk)) return CPK_EDEVICE;
  tc.mark(kTrRWait);
  uint64_t w0, words;
  const int st = rm_info_out(info, h_info, w0, words);
  // (the words chunk by chunk: each chunk's copy-out under the next's DMA)
  if (!st && words && stage_out(sl, h_out, (uint64_t *)sl.d_out + w0, words * 8, p->sk)) return CPK_EDEVICE;
  guard.done();
  if (st) return st;
  tc.mark(kTrROut);
  return CPK_OK;
}

int cpk_generate(cpk_ctx ctx, const cpk_gen_params *params, const uint64_t *d_swo, uint32_t n,
                 void *d_out, void *stream) {
  if (!ctx || !params) return CPK_EINVAL;
  if (n == 0) return CPK_OK;
  DeviceGuard g(ctx->device);
  unsigned grid = (n + 255) / 256;
  hipLaunchKernelGGL(cpk::generate_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, *params,
                     d_swo, n, (uint64_t *)d_out);
  return hip_ok(hipGetLastError());
}

int cpk_count_mismatch(cpk_ctx ctx, const void *d_a, const void *d_b, uint64_t words,
                       uint64_t *d_mismatch, void *stream) {
  if (!ctx) return CPK_EINVAL;
  if (words == 0) return CPK_OK;
  DeviceGuard g(ctx->device);
  unsigned grid = (unsigned)(8 * ctx->cus);
  hipLaunchKernelGGL(cpk::mismatch_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream,
                     (const uint64_t *)d_a, (const uint64_t *)d_b, words,
                     (unsigned long long *)d_mismatch);
  return hip_ok(hipGetLastError());
}

}  // extern "C"
