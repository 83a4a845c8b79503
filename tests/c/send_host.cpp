// Host driver of util_amd/csrc/ws_send.h (tests/test_send_host.py): the header's sequential
// connection routine, the same connection computed the way the kernels do (runs of slots
// summarised, the summaries folded, every message placed by the fold of what lies before it, its
// bytes taken from ws_send_byte), the closed-form lengths and the workspace layout. Built as a
// shared library for ctypes and, with -DSEND_HOST_MAIN, as a program of its own that replays a
// file of cases (written by the test) under a set of capacities: the build for sanitizers.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../util_amd/csrc/ws_send.h"

extern "C" {

long long ws_send_host_connection(const unsigned char* src, uint64_t src_len, const WebsocketSendMsg_t* msg, uint32_t nmsg,
                                  uint32_t F, const uint32_t* keys, unsigned char* tx, uint64_t cap, uint64_t* moff,
                                  WebsocketSendResult_t* out) {
    return (long long)ws_send_connection(src, src_len, msg, nmsg, F, keys, tx, cap, moff, out);
}

// The connection in runs: run r holds the slots [cut[r-1], cut[r]) (cut[-1] = 0, the last run ends
// at nmsg; cuts past nmsg are nmsg).
long long ws_send_host_runs(const unsigned char* src, uint64_t src_len, const WebsocketSendMsg_t* msg, uint32_t nmsg,
                            uint32_t F, const uint32_t* keys, unsigned char* tx, uint64_t cap, uint64_t* moff,
                            WebsocketSendResult_t* out, const uint32_t* cut, uint32_t ncut) {
    const uint32_t role = keys ? 1u : 0u, shard = ws_send_shard(F, role);
    std::vector<uint32_t> lo(ncut + 2);
    lo[0] = 0;
    for (uint32_t r = 0; r < ncut; ++r) lo[r + 1] = cut[r] < nmsg ? cut[r] : nmsg;
    lo[ncut + 1] = nmsg;
    std::vector<WsSendSum> run(ncut + 1), excl(ncut + 1);
    for (uint32_t r = 0; r <= ncut; ++r) {
        run[r] = ws_send_sum_none();
        for (uint32_t i = lo[r]; i < lo[r + 1]; ++i) run[r] = ws_send_comb(run[r], ws_send_sum_msg(msg[i], i, src_len, F, role));
    }
    WsSendSum all = ws_send_sum_none();
    for (uint32_t r = 0; r <= ncut; ++r) {
        excl[r] = all;
        all = ws_send_comb(all, run[r]);
    }
    *out = ws_send_result(all);
    const bool ok = out->status == WEBSOCKET_SEND_OK;
    for (uint32_t r = 0; r <= ncut; ++r) {
        WsSendSum before = excl[r];
        for (uint32_t i = lo[r]; i < lo[r + 1]; ++i) {
            const WsSendSum mine = ws_send_sum_msg(msg[i], i, src_len, F, role);
            WsSendRec rec = {ok ? before.bytes : 0ull, msg[i].src_off, msg[i].len, ok && mine.nmsg ? mine.bytes : 0ull, shard,
                             keys ? keys[i] : 0u, msg[i].type, role};
            if (moff) moff[i] = rec.tx_off;
            for (uint64_t p = 0; p < rec.wire && rec.tx_off + p < cap; ++p) tx[rec.tx_off + p] = ws_send_byte(rec, src, p);
            before = ws_send_comb(before, mine);
        }
    }
    return (long long)out->tx_len;
}

// (a op b) op c == a op (b op c) for the runs [0, na), [na, na + nb), [na + nb, n) of msg; 0: equal
uint32_t ws_send_host_assoc(const WebsocketSendMsg_t* msg, uint32_t na, uint32_t nb, uint32_t nc, uint64_t src_len, uint32_t F,
                            uint32_t role) {
    auto fold = [&](uint32_t lo, uint32_t hi) {
        WsSendSum s = ws_send_sum_none();
        for (uint32_t i = lo; i < hi; ++i) s = ws_send_comb(s, ws_send_sum_msg(msg[i], i, src_len, F, role));
        return s;
    };
    const WsSendSum a = fold(0, na), b = fold(na, na + nb), c = fold(na + nb, na + nb + nc);
    const WsSendSum l = ws_send_comb(ws_send_comb(a, b), c), r = ws_send_comb(a, ws_send_comb(b, c));
    return (uint32_t)(l.first_bad != r.first_bad || (l.first_bad != WS_SEND_NONE && l.status != r.status) || l.nmsg != r.nmsg ||
                      l.bytes != r.bytes || l.frames != r.frames);
}

// out: {shard, frames, wire}; returns 0 where the rule refuses (a body and no shard)
uint32_t ws_send_host_geo(uint64_t L, uint32_t F, uint32_t role, uint64_t* out) {
    const uint32_t shard = ws_send_shard(F, role);
    out[0] = shard;
    if (L && !shard) return 0;
    const WsSendGeo g = ws_send_geo(L, shard, role);
    out[1] = g.frames;
    out[2] = g.wire;
    return 1;
}

uint32_t ws_send_host_frag_key(uint32_t key, uint64_t j) { return ws_send_frag_key(key, j); }

void ws_send_host_layout(uint32_t nseg, uint32_t max_msgs, uint64_t cap, uint64_t* out) {
    const WsSendLayout L = ws_send_layout(nseg, max_msgs, cap);
    const uint64_t v[10] = {L.bo64, L.loc, L.tail, L.agg, L.rec, L.ptr, L.bytes, L.nb, L.ntiles, L.npieces};
    memcpy(out, v, sizeof(v));
}
uint64_t ws_send_host_pieces(uint64_t limit, uint32_t lead) { return ws_send_pieces(limit, lead); }
uint32_t ws_send_host_sizes() {
    return (uint32_t)(sizeof(WsSendSum) | sizeof(WsSendRec) << 8 | sizeof(WebsocketSendResult_t) << 16 |
                      sizeof(WebsocketSendMsg_t) << 24);
}
}

#ifdef SEND_HOST_MAIN
// The case file (little-endian): the number of cases (u32), then per case 6 u32 words {src bytes,
// nmsg, F, has keys, expected tx bytes, expected status}, the source, nmsg entries, nmsg keys when
// there are keys, the expected wire bytes.
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
    T* many(size_t n) {                                  // exactly n elements: a read past them is the sanitizer's
        T* v = (T*)malloc(n ? n * sizeof(T) : 1);
        ok = ok && (n == 0 || fread(v, sizeof(T), n, f) == n);
        return v;
    }
};

int main(int argc, char** argv) {
    if (argc < 2) {
        printf("usage: send_host CASEFILE\n");
        return 2;
    }
    Reader in{fopen(argv[1], "rb")};
    if (!in.f) return 2;
    const uint32_t ncase = in.get<uint32_t>();
    unsigned long long runs = 0;
    for (uint32_t c = 0; c < ncase && in.ok; ++c) {
        uint32_t w[6];
        for (uint32_t& v : w) v = in.get<uint32_t>();
        const uint32_t nsrc = w[0], nmsg = w[1], F = w[2], nexp = w[4];
        unsigned char* src = in.many<unsigned char>(nsrc);
        WebsocketSendMsg_t* msg = in.many<WebsocketSendMsg_t>(nmsg);
        uint32_t* keys = w[3] ? in.many<uint32_t>(nmsg) : nullptr;
        unsigned char* exp = in.many<unsigned char>(nexp);
        if (!in.ok) break;
        // capacities around 0, the header edges and the end; sequentially and cut into two runs
        std::vector<uint64_t> caps = {0, 1, 2, 3, 5, 7, 11, 15, 16, 17};
        for (uint64_t d = 0; d < 3; ++d) {
            if (nexp >= d) caps.push_back(nexp - d);
            caps.push_back(nexp / 2 + d);
        }
        caps.push_back((uint64_t)nexp + 1);
        for (uint64_t cap : caps) {
            for (uint32_t cut = 0; cut <= nmsg + 1; ++cut) {
                unsigned char* tx = (unsigned char*)malloc(cap ? cap : 1);
                memset(tx, 0xEE, cap ? cap : 1);
                uint64_t* moff = (uint64_t*)malloc(nmsg ? nmsg * 8 : 1);
                WebsocketSendResult_t out;
                memset(&out, 9, sizeof(out));
                const long long len = cut == nmsg + 1 ? ws_send_host_connection(src, nsrc, msg, nmsg, F, keys, cap ? tx : nullptr,
                                                                                cap, moff, &out)
                                                      : ws_send_host_runs(src, nsrc, msg, nmsg, F, keys, cap ? tx : nullptr, cap,
                                                                          moff, &out, &cut, 1);
                const uint64_t fit = cap < nexp ? cap : nexp;
                if (len != (long long)nexp || out.status != w[5] || out.tx_len != nexp || memcmp(tx, exp, fit) != 0) {
                    printf("case %u cap %llu cut %u: length %lld (expected %u), status %u (expected %u)\n", c,
                           (unsigned long long)cap, cut, len, nexp, out.status, w[5]);
                    return 1;
                }
                free(tx);
                free(moff);
                ++runs;
            }
        }
        free(src);
        free(msg);
        free(keys);
        free(exp);
    }
    if (!in.ok) {
        printf("short case file\n");
        return 2;
    }
    fclose(in.f);
    printf("send_host ok: %u cases, %llu runs\n", ncase, runs);
    return 0;
}
#endif
