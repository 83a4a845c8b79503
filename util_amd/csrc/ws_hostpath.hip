// ws_hostpath.hip — websocketframeBatchDecodeHost: the batch lives in host memory
// (the reactor's inbufs, net_reactor.c:484-498). Pipelined over groups of
// consecutive segments on WS_HOST_SLOTS streams, each with its own device slot:
//   H2D(group g+2) | decode(group g+1) | D2H(group g)
// so the PCIe copies in both directions and the kernel overlap. With pinned host
// memory (hipHostMalloc / hipHostRegister) the copies are asynchronous DMA; pageable
// memory works but goes through the runtime's staging copies.
//
// The device slot is addressed as d_slot - lo, so the kernel sees the caller's own
// segment offsets and writes descriptors with buffer-relative offsets directly.
// Only segment bytes are copied back (adjacent segments merged into one copy): host bytes
// between segments are read by the H2D copy of a group's span but never written, so a
// neighbouring inbuf that another thread is filling meanwhile is left alone. The calling
// thread's current HIP device is restored before returning.
#include <algorithm>
#include <mutex>
#include <thread>
#include <vector>

#include <string>

#include "ws_common.h"
#include "ws_hostplan.h"

#define WS_HOST_DEV 64
#define WS_HOST_SLOTS 3

struct WsHostSlot {
    hipStream_t st = nullptr;
    unsigned char* buf = nullptr;
    size_t buf_bytes = 0;
    u64* segs = nullptr;  // seg_off[cap] then seg_len[cap]
    size_t seg_cap = 0;
    WebsocketFrameDesc_t* desc = nullptr;
    size_t desc_cap = 0;
    WebsocketSegResult_t* res = nullptr;
    size_t res_cap = 0;
    unsigned char* ws = nullptr;   // decode workspace of this slot's stream
    size_t ws_cap = 0;
};

struct WsHostPipe {
    std::mutex mu;
    WsHostSlot slot[WS_HOST_SLOTS];
};
static WsHostPipe g_pipe[WS_HOST_DEV];

std::atomic<size_t> ws_host_chunk_bytes{64ull << 20};  // group size target ("host_chunk_mb")

template <typename T>
static int grow(T** p, size_t* cap, size_t need, const char* what) {
    if (*cap >= need) return 0;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(p), need * sizeof(T));
    if (e != hipSuccess) return ws_set_err(what, e);
    *cap = need;
    return 0;
}

std::atomic<unsigned long long> ws_stat_host_groups{0};   // groups launched by host decodes (since load)

static_assert(sizeof(WebsocketFrameDesc_t) == WS_HOSTPLAN_DESC_BYTES, "ws_hostplan.h counts descriptors of this size");

struct DeviceGuard {          // restores the calling thread's current device on every return
    int dev = -1;
    DeviceGuard() { if (hipGetDevice(&dev) != hipSuccess) dev = -1; }
    ~DeviceGuard() { if (dev >= 0) (void)hipSetDevice(dev); }
};

extern "C" WSFRAME_AMD_EXPORT int websocketframeBatchDecodeHost(unsigned char* h_buf, unsigned long long buflen,
                                                                const u64* h_seg_off, const u64* h_seg_len,
                                                                unsigned int nseg, unsigned int max_frames,
                                                                WebsocketFrameDesc_t* h_desc,
                                                                WebsocketSegResult_t* h_res, int device) {
    if (nseg == 0) return 0;
    if (!h_buf || !h_seg_off || !h_seg_len || !h_desc || !h_res || max_frames == 0)
        return ws_set_msg("websocketframeBatchDecodeHost: invalid argument");
    if (device < 0 || device >= WS_HOST_DEV)
        return ws_set_err("websocketframeBatchDecodeHost: device index", hipErrorInvalidDevice);
    DeviceGuard guard;
    hipError_t e;
    if ((e = hipSetDevice(device)) != hipSuccess) return ws_set_err("hipSetDevice", e);

    // groups of consecutive, ascending, non-overlapping segments of about one chunk, any other
    // layout one group; the host ranges written back per group (ws_hostplan.h)
    const WsHostPlan plan = ws_host_plan(h_seg_off, h_seg_len, nseg, max_frames, buflen, ws_host_chunk_bytes);
    if (plan.outside) return ws_set_msg("websocketframeBatchDecodeHost: segment outside buffer");
    const std::vector<WsHostGroup>& groups = plan.groups;
    std::vector<std::vector<std::pair<uint64_t, uint64_t>>> back(groups.size());
    for (size_t gi = 0; gi < groups.size(); ++gi)
        ws_host_back_ranges(h_seg_off, h_seg_len, groups[gi], plan.ordered, back[gi]);
    const size_t max_span = plan.max_span, max_nseg = plan.max_nseg;
    // the decode picks its path per group (ws_decode_range): the slots' workspace is the largest any
    // group asks for, so no group outgrows its slot's workspace or falls through to the stream's
    size_t wsb = 0;
    for (const WsHostGroup& g : groups)
        wsb = std::max(wsb, ws_decode_workspace_bytes(g.hi - g.lo, g.s1 - g.s0, max_frames));

    WsHostPipe& P = g_pipe[device];
    std::lock_guard<std::mutex> lock(P.mu);
    int rc = 0;
    const int nslots = groups.size() < WS_HOST_SLOTS ? (int)groups.size() : WS_HOST_SLOTS;
    for (int k = 0; k < nslots; ++k) {
        WsHostSlot& S = P.slot[k];
        if (!S.st && (e = hipStreamCreateWithFlags(&S.st, hipStreamNonBlocking)) != hipSuccess)
            return ws_set_err("hipStreamCreate", e);
        if ((e = hipStreamSynchronize(S.st)) != hipSuccess) return ws_set_err("hipStreamSynchronize", e);
        if ((rc = grow(&S.buf, &S.buf_bytes, max_span + WEBSOCKET_BATCH_PAD, "hipMalloc(host slot)"))) return rc;
        if ((rc = grow(&S.segs, &S.seg_cap, 2 * max_nseg, "hipMalloc(host slot segs)"))) return rc;
        if ((rc = grow(&S.desc, &S.desc_cap, max_nseg * max_frames, "hipMalloc(host slot desc)"))) return rc;
        if ((rc = grow(&S.res, &S.res_cap, max_nseg, "hipMalloc(host slot res)"))) return rc;
        if (wsb && S.ws_cap < wsb) {
            if ((rc = grow(&S.ws, &S.ws_cap, wsb, "hipMalloc(host slot workspace)"))) return rc;
            if ((e = hipMemset(S.ws, 0, 16)) != hipSuccess) return ws_set_err("hipMemset(host slot workspace)", e);
        }
    }
#define WS_TRY(call, what) do { if ((e = (call)) != hipSuccess) { rc = ws_set_err(what, e); goto drain; } } while (0)
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        const WsHostGroup& g = groups[gi];
        WsHostSlot& S = P.slot[gi % nslots];
        const u32 n = g.s1 - g.s0;
        const size_t span = g.hi - g.lo;
        const size_t nd = (size_t)n * max_frames;
        WS_TRY(hipMemcpyAsync(S.buf, h_buf + g.lo, span, hipMemcpyHostToDevice, S.st), "H2D batch");
        WS_TRY(hipMemsetAsync(S.buf + span, 0, WEBSOCKET_BATCH_PAD, S.st), "hipMemset(pad)");
        WS_TRY(hipMemcpyAsync(S.segs, h_seg_off + g.s0, n * sizeof(u64), hipMemcpyHostToDevice, S.st), "H2D seg_off");
        WS_TRY(hipMemcpyAsync(S.segs + S.seg_cap / 2, h_seg_len + g.s0, n * sizeof(u64), hipMemcpyHostToDevice, S.st),
               "H2D seg_len");
        WS_TRY(hipMemsetAsync(S.desc, 0, nd * sizeof(WebsocketFrameDesc_t), S.st), "hipMemset(desc)");
        rc = ws_decode_range(S.buf - g.lo, g.lo, g.hi, S.segs, S.segs + S.seg_cap / 2, n, max_frames, nullptr, S.desc,
                             S.res, S.st, S.ws, S.ws_cap);
        if (rc) goto drain;
        ++ws_stat_host_groups;
        for (const auto& x : back[gi])
            WS_TRY(hipMemcpyAsync(h_buf + x.first, S.buf + (x.first - g.lo), x.second - x.first, hipMemcpyDeviceToHost,
                                  S.st), "D2H batch");
        WS_TRY(hipMemcpyAsync(h_desc + (size_t)g.s0 * max_frames, S.desc, nd * sizeof(WebsocketFrameDesc_t),
                              hipMemcpyDeviceToHost, S.st), "D2H desc");
        WS_TRY(hipMemcpyAsync(h_res + g.s0, S.res, n * sizeof(WebsocketSegResult_t), hipMemcpyDeviceToHost, S.st),
               "D2H res");
    }
#undef WS_TRY
drain:
    for (int k = 0; k < nslots; ++k) {
        hipError_t e2 = hipStreamSynchronize(P.slot[k].st);
        if (e2 != hipSuccess && !rc) rc = ws_set_err("hipStreamSynchronize", e2);
    }
    return rc;
}

// ---------------------------------------------------------------------------------------------
// Several devices on one host rx arena (net_reactor.c:484-500): the
// ascending segments are cut into `ndev` contiguous ranges of about equal bytes (the segment
// boundary nearest to each equal share), and each range runs websocketframeBatchDecodeHost's
// pipeline on its own device from its own host thread, so every device's PCIe link carries its
// share (one pinned arena served by up to ndev links). A device listed twice runs its ranges one
// after the other (its pipeline is locked per device). Any other segment layout is decoded on
// devices[0] alone. A device index or a segment out of range fails the call before any range
// runs; otherwise it returns the first range's error (every range is drained first).
extern "C" WSFRAME_AMD_EXPORT int websocketframeBatchDecodeHostMulti(unsigned char* h_buf, unsigned long long buflen,
                                                                     const u64* h_seg_off, const u64* h_seg_len,
                                                                     unsigned int nseg, unsigned int max_frames,
                                                                     WebsocketFrameDesc_t* h_desc,
                                                                     WebsocketSegResult_t* h_res, const int* devices,
                                                                     int ndev) {
    if (nseg == 0) return 0;
    if (!devices || ndev <= 0 || !h_seg_off || !h_seg_len)
        return ws_set_msg("websocketframeBatchDecodeHostMulti: invalid argument");
    // what no range may find out after another has written its results: a device index or a segment
    // out of range fails the whole call before anything runs
    for (int r = 0; r < ndev; ++r)
        if (devices[r] < 0 || devices[r] >= WS_HOST_DEV) {
            char msg[160];
            snprintf(msg, sizeof(msg), "websocketframeBatchDecodeHostMulti (device %d): device index: %s", devices[r],
                     hipGetErrorString(hipErrorInvalidDevice));
            ws_set_msg(msg);
            return -(int)hipErrorInvalidDevice;
        }
    if (!ws_host_inside(h_seg_off, h_seg_len, nseg, buflen))
        return ws_set_msg("websocketframeBatchDecodeHostMulti: segment outside buffer");
    if (ws_host_multi_single(ws_host_ordered(h_seg_off, h_seg_len, nseg), nseg, ndev))
        return websocketframeBatchDecodeHost(h_buf, buflen, h_seg_off, h_seg_len, nseg, max_frames, h_desc, h_res,
                                             devices[0]);
    // cuts: the segment boundary nearest to each equal share of the bytes (ws_hostplan.h)
    const std::vector<u32> cut = ws_host_cuts(h_seg_len, nseg, ndev);
    const u32 nd = (u32)cut.size() - 1;
    std::vector<int> rc(nd, 0);
    std::vector<std::string> err(nd);
    auto part = [&](u32 r) {
        const u32 a = cut[r], b = cut[r + 1];
        if (a < b) {
            rc[r] = websocketframeBatchDecodeHost(h_buf, buflen, h_seg_off + a, h_seg_len + a, b - a, max_frames,
                                                  h_desc + (size_t)a * max_frames, h_res + a, devices[r]);
            if (rc[r]) err[r] = websocketframeGpuLastError();            // (the error text is per thread)
        }
    };
    std::vector<std::thread> th;
    th.reserve(nd);
    for (u32 r = 1; r < nd; ++r) th.emplace_back(part, r);
    part(0);
    for (auto& t : th) t.join();
    for (u32 r = 0; r < nd; ++r)
        if (rc[r]) {
            char msg[320];
            snprintf(msg, sizeof(msg), "websocketframeBatchDecodeHostMulti (device %d): %s", devices[r], err[r].c_str());
            ws_set_msg(msg);
            return rc[r];
        }
    return 0;
}
