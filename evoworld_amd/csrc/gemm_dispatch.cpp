// gemm_dispatch.cpp -- host front end of ew_gemm_f16: argument validation, routing over the kernel families, the epilogue-variant
// selection of generations 2 / 3 and the stream-K workspace pool of generation 3.  No device code.
#include "gemm_common.h"
#include <mutex>

static int g_gemm_gen = -1;
static int g_gemm_dbg = 0;
static char g_gemm_last_kernel[64] = "";          // rocprof-style name of the kernel the last ew_gemm_f16 call launched
extern "C" const char* ew_gemm_last_kernel(void) { return g_gemm_last_kernel; }
extern "C" void ew_set_gemm_debug(int d) { g_gemm_dbg = d; }
extern "C" void ew_set_gemm_generation(int gen) { g_gemm_gen = gen; }
extern "C" int ew_get_gemm_generation(void) { return g_gemm_gen < 0 ? (g_gemm_gen = 3) : g_gemm_gen; }
void ew_gemm_note_kernel(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_gemm_last_kernel, sizeof(g_gemm_last_kernel), fmt, ap);
    va_end(ap);
}

extern "C" int ew_gemm_convup2_ok(int N, int C) { return N > 0 && N % 320 == 0 && C > 0 && C % 64 == 0; }

// operand sets that occur in the U-Net (evoworld_amd/unet.py); any other mask runs on the smallest compiled superset
ew_status ew_gemm_select_epi(const GemmP& p, int generation, int* epi) {
    const bool dense = p.mode == EW_A_DENSE;
    if (p.act == EW_ACT_GEGLU && !dense) { ew_set_error("ew_gemm_f16: GEGLU epilogue is only built for dense mode"); return EW_ERR_UNSUPPORTED; }
    if (p.act == EW_ACT_GEGLU) { *epi = 8; return EW_OK; }
    const int mask = (p.rowbias ? 1 : 0) | (p.r1 ? 2 : 0) | (p.r2 ? 4 : 0);
    if (p.r1_lo || p.r2_lo || p.out_lo) {           // split-fp16 residual stream: general path with the lo companions
        // generation 3 only, no residual operand (round 5): the row-bias enters through the accumulators' initial value, the epilogue
        // only converts and stores
        if (generation >= 3 && (mask & 6) == 0) *epi = 16 | 1;
        else if (dense) *epi = (mask & 4) == 0 ? 16 | 3 : 16 | 7;
        else if ((mask & 5) == 0) *epi = 16 | 2;
        // row-bias + split output (round 3: the conv1 / temporal conv1 outputs of the resblocks, GroupNorm inputs whose fp16
        // rounding was the largest remaining storage term of the parity budget); r1 may be null (zero page)
        else if ((mask & 4) == 0) *epi = 16 | 3;
        else { ew_set_error("ew_gemm_f16: conv modes carry the split residual with row-bias / r1 only (no r2)"); return EW_ERR_UNSUPPORTED; }
        return EW_OK;
    }
    if (mask <= 2 || (dense && mask == 3)) *epi = mask;
    else *epi = dense && (mask == 6 || mask == 4) ? 6 : 7;
    return EW_OK;
}

extern "C" ew_status ew_gemm_f16(const ew_gemm_args* a, void* stream) {
    EW_REQUIRE(a != nullptr, "ew_gemm_f16: null args");
    EW_REQUIRE(a->a && a->w && a->out && a->zero_page, "ew_gemm_f16: null a/w/out/zero_page");
    EW_REQUIRE(a->M > 0 && a->N > 0, "ew_gemm_f16: M,N must be > 0 (M=%d N=%d)", a->M, a->N);
    EW_REQUIRE(a->c1 > 0 && a->c1 % 64 == 0 && a->c2 >= 0 && a->c2 % 64 == 0,
               "ew_gemm_f16: c1,c2 must be multiples of 64 (c1=%d c2=%d)", a->c1, a->c2);
    EW_REQUIRE(a->c2 == 0 || a->a2, "ew_gemm_f16: c2 > 0 needs a2");
    EW_REQUIRE(a->N % 4 == 0 && a->ld_out % 4 == 0, "ew_gemm_f16: N and ld_out must be multiples of 4");
    EW_REQUIRE(a->lda % 8 == 0 && (a->c2 == 0 || a->lda2 % 8 == 0), "ew_gemm_f16: lda must be a multiple of 8");
    EW_REQUIRE(a->rows_per_group >= 1, "ew_gemm_f16: rows_per_group must be >= 1");
    EW_REQUIRE(!a->r1 || a->ld_r1 % 4 == 0, "ew_gemm_f16: ld_r1 must be a multiple of 4");
    EW_REQUIRE(!a->r2 || a->ld_r2 % 4 == 0, "ew_gemm_f16: ld_r2 must be a multiple of 4");
    int taps = 1;
    if (a->mode == EW_A_CONV3X3) {
        taps = 9;
        EW_REQUIRE(a->n_img > 0 && a->h_in > 0 && a->w_in > 0 && a->h_out > 0 && a->w_out > 0 &&
                       (a->stride == 1 || a->stride == 2) && (a->upsample >= 0 && a->upsample <= 2),
                   "ew_gemm_f16: bad conv3x3 geometry");
        EW_REQUIRE((long long)a->n_img * a->h_out * a->w_out == a->M, "ew_gemm_f16: M != n_img*h_out*w_out");
        EW_REQUIRE(!(a->upsample && a->stride != 1), "ew_gemm_f16: upsample needs stride 1");
        EW_REQUIRE((a->conv_shift == 0 || a->conv_shift == 1) && !(a->conv_shift && a->upsample), "ew_gemm_f16: conv_shift must be 0 or 1 (not with upsample)");
        if (a->upsample == 2) {      // four 2x2 phase convs over the source image, w in the phase pack (evoworld_hip.h)
            EW_REQUIRE(!a->a2 && a->c2 == 0, "ew_gemm_f16: upsample = 2 reads one source (no a2 / c2)");
            EW_REQUIRE(a->h_out == 2 * a->h_in && a->w_out == 2 * a->w_in, "ew_gemm_f16: upsample = 2 needs h_out = 2 h_in and w_out = 2 w_in (got %dx%d -> %dx%d)",
                       a->h_in, a->w_in, a->h_out, a->w_out);
            EW_REQUIRE(!a->rowbias && !a->r1 && !a->r2 && a->act == EW_ACT_NONE, "ew_gemm_f16: upsample = 2 is bias + (split) output only: no rowbias / r1 / r2 / act");
            EW_REQUIRE(ew_gemm_convup2_ok(a->N, a->c1), "ew_gemm_f16: upsample = 2 runs on generation 3's 256x320 tile only: N %% 320 == 0 (N=%d c1=%d)", a->N, a->c1);
        }
    } else if (a->mode == EW_A_CONVT3) {
        taps = 3;
        EW_REQUIRE(a->tB > 0 && a->tT > 0 && a->tP > 0 && (long long)a->tB * a->tT * a->tP == a->M,
                   "ew_gemm_f16: M != B*T*P");
    } else {
        EW_REQUIRE(a->mode == EW_A_DENSE, "ew_gemm_f16: unknown mode %d", a->mode);
    }
    EW_REQUIRE(a->act == EW_ACT_NONE || a->act == EW_ACT_SILU || a->act == EW_ACT_GEGLU || a->act == EW_ACT_GELU, "ew_gemm_f16: unknown act %d", a->act);
    EW_REQUIRE(!a->rowbias || a->ld_rowbias % 4 == 0, "ew_gemm_f16: ld_rowbias must be a multiple of 4");
    if (a->act == EW_ACT_GEGLU)
        EW_REQUIRE(a->N % 128 == 0 && !a->rowbias && !a->r1 && !a->r2 && !a->out_lo, "ew_gemm_f16: GEGLU needs N %% 128 == 0 and no residuals");
    EW_REQUIRE((!a->r1_lo || a->r1) && (!a->r2_lo || a->r2), "ew_gemm_f16: r1_lo / r2_lo need r1 / r2");
    GemmP p;
    p.a = (const f16*)a->a; p.a2 = (const f16*)a->a2; p.w = (const f16*)a->w; p.bias = (const f16*)a->bias;
    p.rowbias = (const f16*)a->rowbias; p.r1 = (const f16*)a->r1; p.r2 = (const f16*)a->r2; p.out = (f16*)a->out;
    p.zero_page = (const f16*)a->zero_page;
    p.r1_lo = (const int8_t*)a->r1_lo; p.r2_lo = (const int8_t*)a->r2_lo; p.out_lo = (int8_t*)a->out_lo;
    p.conv_shift = a->conv_shift;
    p.M = a->M; p.N = a->N; p.K = taps * (a->c1 + a->c2);
    p.c1 = a->c1; p.c2 = a->c2; p.lda = a->lda; p.lda2 = a->lda2; p.ld_out = a->ld_out; p.ld_r1 = a->ld_r1; p.ld_r2 = a->ld_r2; p.ld_rowbias = a->ld_rowbias;
    p.mode = a->mode; p.n_img = a->n_img; p.h_in = a->h_in; p.w_in = a->w_in; p.h_out = a->h_out; p.w_out = a->w_out;
    p.stride = a->stride; p.upsample = a->upsample; p.tB = a->tB; p.tT = a->tT; p.tP = a->tP;
    p.rows_per_group = a->rows_per_group; p.act = a->act; p.c_acc = a->c_acc; p.c_r1 = a->c_r1; p.c_r2 = a->c_r2;
    p.tiles_m = p.tiles_n = 0;
    p.band = 0;
    p.dbg = g_gemm_dbg;
    hipStream_t s = (hipStream_t)stream;
    const int gen = ew_get_gemm_generation();
    bool taken = false;
    ew_status st = EW_OK;
    // the four-phase form of the upsample conv has one kernel (generation 3), whichever generation is selected: no other family reads its weight pack
    if (p.mode == EW_A_CONV3X3 && p.upsample == 2) return ew_gemm3_convup2(p, s);
    // 3x3 convs with a handful of output channels (conv_out: N = 4) have their own kernel (round 6); generation 1 stays the independent cross-check
    if (gen >= 2 && ((st = ew_conv_small_n_try(p, s, &taken)) || taken)) return st;
    // generation 3 (256x320 tile, then 256x256) where it applies and fills the chip, generation 2 otherwise
    if (gen >= 3 && ((st = ew_gemm3_try(p, s, &taken)) || taken)) return st;
    if (gen >= 3 && ((st = ew_gemm3_try_b256(p, s, &taken)) || taken)) return st;
    return gen >= 2 ? ew_gemm2_dispatch(p, s) : ew_gemm1_dispatch(p, s);
}

// ---- stream-K workspace pool ----
struct SkDesc { unsigned epoch; int mode, epi, M, N, K; };                   // what a stream-K launch was (named when its hand-over times out)
constexpr int SK_DESC_RING = 1024, SK_SLOTS = 256, SK_POOL = 64;             // SK_POOL: (device, stream) pairs of the whole process
struct SkWorkspace { int dev; hipStream_t stream; float* ws; unsigned* flags; unsigned epoch; SkDesc* ring; };
struct SkPool {
    const SkInstance& inst;
    SkWorkspace pool[SK_POOL];
    int used = 0;
    std::mutex mutex;                                                         // the pool is shared by every host thread
    SkWorkspace* workspace(hipStream_t stream, bool create) {
        std::lock_guard<std::mutex> lock(mutex);
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return nullptr;
        for (int i = 0; i < used; ++i)
            if (pool[i].dev == dev && pool[i].stream == stream) return &pool[i];
        if (!create || used == SK_POOL) return nullptr;                         // pool full: those launches run the whole-tile schedule
        SkWorkspace w{dev, stream, nullptr, nullptr, 0, nullptr};
        // uncached (MTYPE UC) device memory: partials and flags cross XCDs inside one kernel, and the per-XCD L2s are only coherent
        // at kernel boundaries for ordinary allocations
        if (hipExtMallocWithFlags((void**)&w.ws, SK_SLOTS * inst.slot_floats * sizeof(float), hipDeviceMallocUncached) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        if (hipExtMallocWithFlags((void**)&w.flags, 2048 * sizeof(unsigned), hipDeviceMallocUncached) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(w.ws); return nullptr; }
        if (hipMemsetAsync(w.flags, 0, 2048 * sizeof(unsigned), stream) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(w.flags); (void)hipFree(w.ws); return nullptr; }
        w.ring = new SkDesc[SK_DESC_RING]();
        pool[used] = w;
        return &pool[used++];
    }
    // 0 = every hand-over of this instance completed, 1 = a finisher gave up waiting (message set), -1 = HIP error.  Synchronises.
    int status() {
        std::lock_guard<std::mutex> lock(mutex);      // the descriptor ring is written under the same mutex by launching threads
        int bad = 0;
        for (int i = 0; i < used; ++i) {
            SkWorkspace* w = &pool[i];
            unsigned word[2] = {0, 0};
            if (hipMemcpy(word, w->flags + 1024, sizeof(word), hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return -1; }
            if (!word[0]) continue;
            bad = 1;
            const SkDesc d = w->ring[word[1] % SK_DESC_RING];
            if (d.epoch == word[1])
                ew_set_error("stream-K hand-over timed out: %s<%d, %d> M=%d N=%d K=%d (stream-K launch #%u on device %d, stream %p): the output of that launch is invalid",
                         inst.kernel, d.mode, d.epi, d.M, d.N, d.K, word[1], w->dev, (void*)w->stream);
            else
                ew_set_error("stream-K hand-over timed out in stream-K launch #%u on device %d, stream %p (more than %d stream-K launches ago: description no longer kept)",
                         word[1], w->dev, (void*)w->stream, SK_DESC_RING);
        }
        return bad;
    }
};
static SkPool g_sk[2] = {{ew_gemm3_sk}, {ew_gemm3_sk_b256}};

SkWorkspace* ew_sk_workspace(int inst, hipStream_t s) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusNone; }
    return g_sk[inst].workspace(s, cap == hipStreamCaptureStatusNone);
}
void ew_sk_begin(int inst, SkWorkspace* w, int mode, int epi, const GemmP& p, SkP* sk) {
    std::lock_guard<std::mutex> lock(g_sk[inst].mutex);
    const unsigned e = ++w->epoch;
    w->ring[e % SK_DESC_RING] = SkDesc{e, mode, epi, p.M, p.N, p.K};
    sk->ws = w->ws; sk->flags = w->flags; sk->epoch = e;
}

// both tile instances' workspaces of (current device, stream): optional for eager use, required before a capture (evoworld_hip.h)
extern "C" ew_status ew_gemm_streamk_init(void* stream) {
    const bool a = g_sk[0].workspace((hipStream_t)stream, true) != nullptr;
    const bool b = g_sk[1].workspace((hipStream_t)stream, true) != nullptr;
    if (!a || !b) { ew_set_error("ew_gemm_streamk_init: no stream-K workspace for this (device, stream): allocation failed or all 64 process-wide pool entries are in use; launches on it run the whole-tile schedule"); return EW_ERR_HIP; }
    return EW_OK;
}
extern "C" int ew_gemm_streamk_status(void) {
    const int b = g_sk[1].status();
    const int a = b < 0 ? b : g_sk[0].status();
    return a < 0 ? a : (a | b);
}
