// A scalar model of the raw stream's chunk-parallel walk (util_amd/csrc/ws_stream.hip) over a host
// buffer, built only from the plain parts of ws_link.h (records, pools, lookups, rw_link_decide) and
// ws_step.h (the step rule): candidates, window walks, owner walks, the chain through the records,
// and the emit rows expanded into frame offsets. tests/test_link_host.py holds it against the oracle.
// No unmask. The geometry is the caller's, so a test reaches every branch on small streams.
#include <string.h>

#include <vector>

#include "../../util_amd/csrc/ws_link.h"

// counters[]: what the chain did (the test asserts the branch a case is named for)
enum {
    LK_ROWS_GROUP = 0,   // rows: the group walk to the stream's end
    LK_ROWS_OWNER,       // rows with an owner walk
    LK_CHUNK_WALKS,      // chunks without a usable record, walked by the step rule
    LK_CLIPPED,          // rows whose n_par was clipped by max_frames
    LK_OVER,             // rows that went on at the owner's `over` (more frames than staging)
    LK_POOL_S1,          // records taken from a middle chunk's stream-ending pool
    LK_POOL_SLAST,       // ... from the last chunk's
    LK_DEAD,             // entries whose record's owner walk was dead
    LK_SKIPPED,          // chain steps that skipped at least one chunk
    LK_MAX_PREFIX,       // group rows because max_frames is reached in the window prefix
    LK_MAX_REST,         // last rows whose staged frames fit and whose owner walk's rest met max_frames
    LK_NO_WINDOW,        // entries outside their chunk's window
    LK_NCOUNT
};

namespace {
struct Model {
    const unsigned char* buf;
    u64 buf_bytes, len, P, C;
    u32 H, stgn, max_frames;
    bool need_mask;
    u64* offs;
    bool bad;            // a frame slot past max_frames (a model or rule error)
};

// the 16 bytes at pos as the kernels get them: two little-endian u64, past the buffer zeros
void load16(const Model& m, u64 pos, u64& h0, u64& h1) {
    unsigned char b[16] = {0};
    if (pos < m.buf_bytes) memcpy(b, m.buf + pos, m.buf_bytes - pos < 16 ? m.buf_bytes - pos : 16);
    h0 = h1 = 0;
    for (int i = 7; i >= 0; --i) {
        h0 = (h0 << 8) | b[i];
        h1 = (h1 << 8) | b[8 + i];
    }
}

// one speculative step (the kernels' rw_step)
u32 spec_step(const Model& m, u64& pos) {
    if (pos >= m.len || m.len - pos < 2) return 1;
    u64 h0, h1;
    load16(m, pos, h0, h1);
    u32 fl;
    const u32 r = rw_step_hdr(h0, h1, m.len - pos, m.need_mask, fl);
    pos += fl;
    return r;
}

void put(Model& m, u64 slot, u64 pos) {
    if (slot >= m.max_frames) { m.bad = true; return; }
    m.offs[slot] = pos;
}

// The group walk (stream_walk) from (pos, nf) by the step rule: stops before the first frame at or
// past `end` (not ended), or where the stream's walk ends
struct Walk {
    u64 next;
    u32 nf;
    bool ended;
    int status;
};
Walk walk(Model& m, u64 pos, u32 nf, u64 end) {
    for (;;) {
        const bool eval = pos < m.len;
        u64 h0, h1;
        load16(m, eval ? pos : 0, h0, h1);
        const WsHdr h = ws_parse(h0, h1, eval ? m.len - pos : 0);
        int st;
        const u32 code = ws_cand_code(pos, m.len, nf, m.max_frames, h, 0, true, st);
        if (eval && pos >= end) return {pos, nf, false, WEBSOCKET_SEG_OK};   // the next walk's, whatever it is
        if (code == 3) return {pos, nf, true, st};
        if (h.ret != 0) put(m, nf++, pos);                                   // a ret == 0 frame has no descriptor
        if (code == 2) return {pos, nf, true, st};
        pos += (u32)h.ret;
    }
}
}  // namespace

// The walk of [P, len) with nf frames before P, chunks of C bytes from P, windows of H bytes,
// stgn staged offsets per owner. buf[0, buf_bytes) holds the stream and whatever follows it.
// offs[k] = offset of frame k for the frames from nf on; res as the device writes it; trace[2 i],
// trace[2 i + 1] = chunk and RW_LINK_* kind of chain step i. Returns the chain's steps, < 0 on an
// inconsistency of the model itself.
extern "C" int ws_link_host_stream(const unsigned char* buf, u64 buf_bytes, u64 len, u64 P, u32 nf, u64 C, u32 H,
                                   u32 stgn, u32 max_frames, u32 need_mask, u64* offs, WebsocketSegResult_t* res,
                                   u64* counters, u32* trace, u32 trace_cap) {
    Model m = {buf, buf_bytes, len, P, C, H, stgn, max_frames, need_mask != 0, offs, false};
    for (int i = 0; i < LK_NCOUNT; ++i) counters[i] = 0;
    if (P >= len || !C || !H || H > C || !stgn) return -1;
    const u64 nchunks = (len - P + C - 1) / C;
    std::vector<RwRec> recs(nchunks * RW_SLOTS + RW_SLAST);
    std::vector<u32> nrec(nchunks * 4, 0);
    std::vector<unsigned long long> dx(nchunks * RW_D, 0);
    std::vector<RwOwn> own(nchunks * RW_D);
    std::vector<u32> stg(nchunks * RW_D * stgn, 0);
    for (u64 c = 0; c < nchunks; ++c) {
        const u64 cs0 = P + c * C, cend = cs0 + C, wend = cs0 + H;
        // R1 + R2: every plausible window position that survives two headers walks to the window's end
        // (the window's positions: H bytes from the 16-B line of the chunk's first byte, as R1 scans them)
        for (u64 start = cs0; start < (cs0 & ~15ull) + H && start < len; ++start) {
            u64 h0, h1;
            load16(m, start, h0, h1);
            if (!rw_plausible((u32)h0 & 0xFFu, (u32)(h0 >> 8) & 0xFFu, (u32)(h0 >> 16) & 0xFFFFu, m.need_mask)) continue;
            u64 pos = start;
            if (spec_step(m, pos) == 0 && pos < cend && spec_step(m, pos) == 2) continue;
            pos = start;
            u32 cnt = 0, r = 0;
            while (pos < wend && (r = spec_step(m, pos)) == 0) ++cnt;
            if (r == 2) continue;                                            // a wrong start
            if (r == 0) {                                                    // three more plausible headers
                u64 vp = pos;
                u32 vr = 0;
                for (u32 v = 0; v < 3 && vp < cend && (vr = spec_step(m, vp)) == 0; ++v) {
                }
                if (vr == 2) continue;
            }
            const u32 st = r;
            const RwPools pl = rw_pools(c, nchunks, ~0u, ~0u);
            const u32 slot = nrec[4 * c + st]++;
            if (slot < (st ? pl.n1 : pl.n0)) {
                RwRec rr;
                rr.start = (u32)(start - cs0);
                rr.cs = cnt | (st << 31);
                rr.exit = pos;
                recs[(st ? pl.i1 : pl.i0) + slot] = rr;
            }
            if (st) continue;
            for (u32 d = 0; d < RW_D; ++d) {                                 // the first RW_D distinct exits
                unsigned long long& x = dx[c * RW_D + d];
                if (x == 0) x = pos;
                if (x == pos) break;
            }
        }
        // R3: one walk per claimed exit to the chunk's end
        for (u32 d = 0; d < RW_D; ++d) {
            const u64 oi = c * RW_D + d;
            u64 pos = dx[oi];
            if (!pos) continue;
            u32* sl = &stg[oi * stgn];
            u32 nb = 0, r = 0;
            u64 over = 0;
            while (pos < cend) {
                if (nb < stgn) sl[nb] = (u32)(pos - cs0);
                else if (nb == stgn) over = pos;
                if ((r = spec_step(m, pos)) != 0) break;
                ++nb;
                if (nb > RW_MAXSTEPS) { r = 2; break; }
            }
            RwOwn ow;
            ow.exit = pos;
            ow.cs = nb | ((r == 1 ? 1u : 0u) << 31);
            ow.dead = r == 2 ? 1u : 0u;
            ow.over = over;
            ow.pad = 0;
            own[oi] = ow;
        }
    }
    // the chain from P, each row expanded as the emit does
    u64 ent = P, nfc = nf;
    int steps = 0;
    Walk fin = {P, nf, false, WEBSOCKET_SEG_OK};
    for (bool last = false; !last; ++steps) {
        if ((u64)steps > 4 * nchunks + 16) return -2;
        const u64 c = (ent - P) / C, cs0 = P + c * C;
        RwHit r = {false, 0u, 0ull};
        if (c < nchunks && ent - cs0 >= H) ++counters[LK_NO_WINDOW];
        if (c < nchunks && ent - cs0 < H) {
            const RwPools pl = rw_pools(c, nchunks, nrec[4 * c], nrec[4 * c + 1]);
            r = rw_find_rec(recs.data(), pl, (u32)(ent - cs0));
            RwPools p0 = pl;
            p0.n1 = 0;
            if (r.found && !rw_find_rec(recs.data(), p0, (u32)(ent - cs0)).found)
                ++counters[c + 1 == nchunks ? LK_POOL_SLAST : LK_POOL_S1];
        }
        RwOwnHit ow = {~0ull, 0u, 0u, 0ull};
        if (r.found) ow = rw_find_own(dx.data(), own.data(), c, r.exit);
        const RwLinkOut d = rw_link_decide(ent, cs0, nfc, r, ow, stgn, max_frames, len);
        if ((u32)steps < trace_cap) { trace[2 * steps] = (u32)c; trace[2 * steps + 1] = d.kind; }
        if (d.kind == RW_LINK_WALK) {
            if (r.found && !(r.cs >> 31) && ow.oi != ~0ull && ow.dead) ++counters[LK_DEAD];
            ++counters[LK_CHUNK_WALKS];
            fin = walk(m, ent, (u32)nfc, cs0 + C < len ? cs0 + C : len);
            last = fin.ended;
            if (!last && fin.next <= ent) return -3;
            if (!last && (fin.next - P) / C > c + 1) ++counters[LK_SKIPPED];
            ent = fin.next;
            nfc = fin.nf;
            continue;
        }
        const RwRow& t = d.row;
        last = d.last;
        if (d.kind == RW_LINK_GROUP) {
            ++counters[LK_ROWS_GROUP];
            if (!(r.cs >> 31)) ++counters[LK_MAX_PREFIX];
            fin = walk(m, t.ent, (u32)t.nf0, len);
            continue;
        }
        ++counters[LK_ROWS_OWNER];
        walk(m, t.ent, (u32)t.nf0, t.exit_w);                                // the window prefix
        const RwOwn& o = own[t.owner];
        const u32* sl = &stg[t.owner * stgn];
        for (u64 i = 0; i < t.n_par; ++i) put(m, t.nf0 + t.cnt_w + i, t.cs0 + sl[i]);
        const u64 nb = o.cs & 0x7FFFFFFFu, staged = nb < stgn ? nb : stgn;
        if (t.n_par < staged) ++counters[LK_CLIPPED];
        if (t.n_par == staged && t.n_par != nb) ++counters[LK_OVER];
        const u64 next = t.n_par < staged ? t.cs0 + sl[t.n_par] : (t.n_par == nb ? o.exit : o.over);
        const Walk w2 = walk(m, next, (u32)(t.nf0 + t.cnt_w + t.n_par), t.last ? len : o.exit);
        if (last) {
            fin = w2;
            if (t.n_par == staged && w2.status == WEBSOCKET_SEG_MAX_FRAMES) ++counters[LK_MAX_REST];
        } else {
            if (w2.ended || w2.next != d.ent || w2.nf != d.nfc) return -4;   // the records are the loop itself
            if ((d.ent - P) / C > c + 1) ++counters[LK_SKIPPED];
        }
        ent = d.ent;
        nfc = d.nfc;
    }
    if (m.bad) return -5;
    res->consumed = fin.next;
    res->n_frames = fin.nf;
    res->status = fin.status;
    return steps;
}

// The fill of the walk's per-chunk pools on a chunk grid of the caller's: chunks of C bytes from P (the
// last one to len), windows of H bytes, the buffer's first byte at an address of phase `lead` (mod 16:
// R1 scans whole 16-B lines, one wavefront per 4 KiB from the line of the chunk's first byte).
// counts[4 c ..] for chunk c:
//   [0] the most plausible positions any one wavefront span of its window holds (RW_WCAP stages 256)
//   [1] candidates that survive R1's two headers (the chunk's list holds capc)
//   [2] window walks that leave the window and pass R2's extra headers (RW_S0 record slots)
//   [3] distinct window exits among them (RW_D owner walks)
// Returns the number of chunks, -1 on a bad grid.
extern "C" long long ws_link_host_pool_counts(const unsigned char* buf, u64 buf_bytes, u64 len, u64 P, u64 C, u32 H,
                                              u32 lead, u32 need_mask, u32* counts, u64 counts_cap) {
    Model m = {buf, buf_bytes, len, P, C, H, 64, 1, need_mask != 0, nullptr, false};
    if (P >= len || !C || !H || H > C || (H & 4095) || lead > 15) return -1;
    const u64 nchunks = (len - P + C - 1) / C;
    if (nchunks > counts_cap) return -1;
    for (u64 c = 0; c < nchunks; ++c) {
        const u64 cs0 = P + c * C, cend = cs0 + C, wend = cs0 + H;
        // the window's positions as R1 takes them: H bytes from the 16-B line (by address) of the chunk's first byte
        const u64 a0 = ((lead + cs0) & ~15ull);                              // address - (origin - lead)
        u32 wave_max = 0, survivors = 0, n0 = 0;
        std::vector<u64> exits;
        for (u64 w0 = 0; w0 < H; w0 += 4096) {
            u32 in_wave = 0;
            for (u64 q = 0; q < 4096; ++q) {
                const u64 addr = a0 + w0 + q;
                if (addr < lead + cs0 || addr >= lead + len) continue;       // positions inside [cs0, len) only
                const u64 start = addr - lead;
                u64 h0, h1;
                load16(m, start, h0, h1);
                if (!rw_plausible((u32)h0 & 0xFFu, (u32)(h0 >> 8) & 0xFFu, (u32)(h0 >> 16) & 0xFFFFu, m.need_mask)) continue;
                ++in_wave;
                u64 pos = start;
                if (spec_step(m, pos) == 0 && pos < cend && spec_step(m, pos) == 2) continue;
                ++survivors;
                pos = start;
                u32 r = 0;
                while (pos < wend && (r = spec_step(m, pos)) == 0) {
                }
                if (r != 0) continue;                                        // a wrong start, or the stream's walk ends
                u64 vp = pos;
                u32 vr = 0;
                for (u32 v = 0; v < 3 && vp < cend && (vr = spec_step(m, vp)) == 0; ++v) {
                }
                if (vr == 2) continue;
                ++n0;
                bool seen = false;
                for (u64 e : exits) seen = seen || e == pos;
                if (!seen) exits.push_back(pos);
            }
            if (in_wave > wave_max) wave_max = in_wave;
        }
        counts[4 * c] = wave_max;
        counts[4 * c + 1] = survivors;
        counts[4 * c + 2] = n0;
        counts[4 * c + 3] = (u32)exits.size();
    }
    return (long long)nchunks;
}
