// Host driver of util_amd/csrc/ws_reply.h (tests/test_reply_host.py): the header's sequential
// segment routine, the same segment computed the way the kernels do (runs of frames summarised,
// the summaries folded, every PONG placed by the fold of what lies before it), and the workspace
// layout. Built as a shared library for ctypes and, with -DREPLY_HOST_MAIN, as a program of its
// own that replays a file of cases (the directed table, written by the test) under every cut into
// two runs and every capacity: the build for sanitizers.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../util_amd/csrc/ws_reply.h"

extern "C" {

long long ws_reply_host_segment(const unsigned char* buf, uint64_t seg_off, const WebsocketFrameDesc_t* desc,
                                const WebsocketSegResult_t* res, uint32_t max_frames, uint32_t flags,
                                const WebsocketProtoResult_t* pr, uint32_t fail, const uint32_t* keys, uint32_t* state,
                                unsigned char* tx, uint64_t cap, WebsocketReplyResult_t* out) {
    return (long long)ws_reply_segment(buf, seg_off, desc, res, max_frames, flags, pr, fail, keys, state, tx, cap, out);
}

// The segment in runs: run r holds the frames [cut[r-1], cut[r]) (cut[-1] = 0, the last run ends at
// n; cuts past n are n). Pass 1 summarises every run, pass 2 folds the summaries (exclusive), the
// segment's plan comes from the total, pass 3 writes every answered ping at the fold of the runs
// before its own, then of its run's frames before it.
long long ws_reply_host_runs(const unsigned char* buf, uint64_t seg_off, const WebsocketFrameDesc_t* desc,
                             const WebsocketSegResult_t* res, uint32_t max_frames, uint32_t flags,
                             const WebsocketProtoResult_t* pr, uint32_t fail, const uint32_t* keys, uint32_t* state,
                             unsigned char* tx, uint64_t cap, WebsocketReplyResult_t* out, const uint32_t* cut, uint32_t ncut) {
    const uint32_t n = res->n_frames < max_frames ? res->n_frames : max_frames, keyed = keys ? 1u : 0u;
    const uint32_t first_bad = pr ? pr->first_bad : WS_REPLY_NONE, wm = flags & WEBSOCKET_REPLY_WIRE_MASKED;
    const uint64_t seg_end = seg_off + res->consumed;
    std::vector<uint32_t> lo(ncut + 2);
    lo[0] = 0;
    for (uint32_t r = 0; r < ncut; ++r) lo[r + 1] = cut[r] < n ? cut[r] : n;
    lo[ncut + 1] = n;
    auto sum_of = [&](uint32_t k) {
        const WebsocketFrameDesc_t& d = desc[k];
        return ws_reply_consumed(d, seg_end) ? ws_reply_sum_frame(d.type, d.is_fin, d.datalen, k, (uint32_t)(k < first_bad), keyed)
                                             : ws_reply_sum_none();
    };
    std::vector<WsReplySum> run(ncut + 1), excl(ncut + 1);
    for (uint32_t r = 0; r <= ncut; ++r) {
        run[r] = ws_reply_sum_none();
        for (uint32_t k = lo[r]; k < lo[r + 1]; ++k) run[r] = ws_reply_comb(run[r], sum_of(k));
    }
    WsReplySum all = ws_reply_sum_none();
    for (uint32_t r = 0; r <= ncut; ++r) {
        excl[r] = all;
        all = ws_reply_comb(all, run[r]);
    }
    const uint32_t kind = ws_reply_close_kind(all, first_bad, fail);
    uint32_t status = 0, body = 2;
    if (kind == WEBSOCKET_REPLY_CLOSE_PROTOCOL) status = pr->close_status;
    else if (kind == WEBSOCKET_REPLY_CLOSE_CALLER) status = fail;
    else if (kind == WEBSOCKET_REPLY_CLOSE_ECHO) {
        const WebsocketFrameDesc_t& c = desc[all.close];
        if (c.datalen >= 2) status = ws_reply_echo_status(buf + c.data_off, wm && c.masked);
        else body = 0;
    }
    const WsReplySeg g = ws_reply_seg(all, first_bad, state ? *state : 0u, flags, keyed, kind, status, body);
    for (uint32_t r = 0; r <= ncut; ++r) {
        WsReplySum in = ws_reply_sum_none();
        for (uint32_t k = lo[r]; k < lo[r + 1]; ++k) {
            const WebsocketFrameDesc_t& d = desc[k];
            if (ws_reply_consumed(d, seg_end) && ws_reply_answers(g, flags, k, d.type, d.is_fin, d.datalen)) {
                const uint64_t off = (flags & WEBSOCKET_REPLY_LAST_PING_ONLY) ? 0ull : ws_reply_comb(excl[r], in).bytes;
                ws_reply_write(ws_reply_pong(buf, d.data_off, (uint32_t)d.datalen, wm && d.masked, keyed, keyed ? keys[k] : 0u),
                               tx, off, cap);
            }
            in = ws_reply_comb(in, sum_of(k));
        }
    }
    if (g.close_len) {
        ws_reply_write(ws_reply_close(g.close_status, g.close_len - (keyed ? 6u : 2u), keyed, keyed ? keys[max_frames] : 0u), tx,
                       g.pong_bytes, cap);
        if (state) *state |= WEBSOCKET_REPLY_ST_CLOSE_SENT;
    }
    out->n_pong = g.npong;
    out->close_kind = g.close_kind;
    out->close_status = g.close_status;
    out->tx_len = (uint32_t)(g.pong_bytes + g.close_len);
    return (long long)(g.pong_bytes + g.close_len);
}

// (a op b) op c against a op (b op c) for the summaries of three runs of frames given as (type,
// fin, datalen) triples with indices from 0; returns the number of fields that differ
uint32_t ws_reply_host_assoc(const uint32_t* f, uint32_t na, uint32_t nb, uint32_t nc, uint32_t first_bad, uint32_t keyed) {
    WsReplySum s[3] = {ws_reply_sum_none(), ws_reply_sum_none(), ws_reply_sum_none()};
    const uint32_t end[3] = {na, na + nb, na + nb + nc};
    for (uint32_t k = 0, r = 0; k < end[2]; ++k) {
        while (k >= end[r]) ++r;
        s[r] = ws_reply_comb(s[r], ws_reply_sum_frame(f[3 * k], f[3 * k + 1], f[3 * k + 2], k, (uint32_t)(k < first_bad), keyed));
    }
    const WsReplySum x = ws_reply_comb(ws_reply_comb(s[0], s[1]), s[2]), y = ws_reply_comb(s[0], ws_reply_comb(s[1], s[2]));
    return (uint32_t)(x.close != y.close) + (x.npong != y.npong) + (x.last != y.last) + (x.bytes != y.bytes) +
           (x.last_bytes != y.last_bytes);
}

// {bo, loff, bo64, rec, tail, agg, bytes, nb, ntmax} of the workspace
void ws_reply_host_layout(uint32_t nseg, uint32_t max_frames, uint64_t out[9]) {
    const WsReplyLayout L = ws_reply_layout(nseg, max_frames);
    const uint64_t v[9] = {L.bo, L.loff, L.bo64, L.rec, L.tail, L.agg, L.bytes, L.nb, L.ntmax};
    memcpy(out, v, sizeof(v));
}

uint32_t ws_reply_host_sizes() { return (uint32_t)(sizeof(WsReplySum) | sizeof(WsReplyRec) << 8 | sizeof(WebsocketReplyResult_t) << 16); }

}  // extern "C"

#ifdef REPLY_HOST_MAIN
// The case file (little-endian u32 words unless said otherwise): the number of cases, then per case
// 15 words {wire bytes, max_frames, flags, has proto, first_bad, proto status, fail, has keys,
// state (0xFFFFFFFF: none), reply bytes, n_pong, close_kind, close_status, tx_len, state out},
// seg_off (u64), the wire, max_frames descriptors, the segment result, max_frames + 1 keys when
// there are keys, the expected reply.
struct Reader {
    FILE* f;
    bool ok = true;
    template <typename T>
    T get() {
        T v{};
        ok = ok && fread(&v, sizeof(T), 1, f) == 1;
        return v;
    }
    template <typename T>
    std::vector<T> many(size_t n) {
        std::vector<T> v(n ? n : 1);
        ok = ok && (n == 0 || fread(v.data(), sizeof(T), n, f) == n);
        return v;
    }
};

int main(int argc, char** argv) {
    if (argc < 2) {
        printf("usage: reply_host CASEFILE\n");
        return 2;
    }
    Reader in{fopen(argv[1], "rb")};
    if (!in.f) return 2;
    const uint32_t ncase = in.get<uint32_t>();
    unsigned long long runs = 0;
    for (uint32_t c = 0; c < ncase && in.ok; ++c) {
        uint32_t w[15];
        for (uint32_t& v : w) v = in.get<uint32_t>();
        const uint64_t seg_off = in.get<uint64_t>();
        const uint32_t mf = w[1], flags = w[2], fail = w[6], nexp = w[9];
        const std::vector<unsigned char> wire = in.many<unsigned char>(w[0]);
        const std::vector<WebsocketFrameDesc_t> desc = in.many<WebsocketFrameDesc_t>(mf);
        const WebsocketSegResult_t res = in.get<WebsocketSegResult_t>();
        const std::vector<uint32_t> keys = in.many<uint32_t>(w[7] ? mf + 1 : 0);
        const std::vector<unsigned char> exp = in.many<unsigned char>(nexp);
        if (!in.ok) break;
        const WebsocketProtoResult_t pr = {w[4], 0u, w[5], WS_REPLY_NONE};
        const uint32_t n = res.n_frames < mf ? res.n_frames : mf;
        // every capacity 0..nexp + 1 (exactly `cap` bytes allocated: a write past it is the sanitizer's),
        // sequentially and under every cut into two runs
        for (uint32_t cap = 0; cap <= nexp + 1; ++cap) {
            for (uint32_t cut = 0; cut <= n + 1; ++cut) {
                unsigned char* tx = (unsigned char*)malloc(cap ? cap : 1);
                memset(tx, 0xEE, cap ? cap : 1);
                uint32_t st = w[8];
                WebsocketReplyResult_t out = {9, 9, 9, 9};
                const long long len =
                    cut == n + 1 ? ws_reply_host_segment(wire.data(), seg_off, desc.data(), &res, mf, flags, w[3] ? &pr : nullptr,
                                                         fail, w[7] ? keys.data() : nullptr, w[8] == WS_REPLY_NONE ? nullptr : &st,
                                                         cap ? tx : nullptr, cap, &out)
                                 : ws_reply_host_runs(wire.data(), seg_off, desc.data(), &res, mf, flags, w[3] ? &pr : nullptr, fail,
                                                      w[7] ? keys.data() : nullptr, w[8] == WS_REPLY_NONE ? nullptr : &st,
                                                      cap ? tx : nullptr, cap, &out, &cut, 1);
                const uint32_t fit = cap < nexp ? cap : nexp;
                bool ok = len == (long long)nexp && memcmp(tx, exp.data(), fit) == 0 && out.n_pong == w[10] &&
                          out.close_kind == w[11] && out.close_status == w[12] && out.tx_len == w[13] &&
                          (w[8] == WS_REPLY_NONE || st == w[14]);
                for (uint32_t i = fit; i < cap; ++i) ok = ok && tx[i] == 0xEE;
                free(tx);
                if (!ok) {
                    printf("reply_host: case %u capacity %u cut %u disagrees with the table\n", c, cap, cut);
                    return 1;
                }
                ++runs;
            }
        }
    }
    fclose(in.f);
    if (!in.ok) {
        printf("reply_host: short case file\n");
        return 2;
    }
    printf("reply_host ok: %u cases, %llu runs\n", ncase, runs);
    return 0;
}
#endif
