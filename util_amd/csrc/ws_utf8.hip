// ws_utf8.hip — websocketframeBatchValidateTextDevice (include/wsframe_amd_text.h): UTF-8
// validation of reassembled text messages and CLOSE reasons, for gfx950. The byte rule, the
// unfinished tail and the state word are ws_utf8.h's (one definition, host-tested).
//
// Work is divided by bytes. The host knows no sizes, so the plan is made on the device (the block
// sum, the offsets scan and the wave search are ws_scan.h's, one definition):
//   plan    one thread per message slot: class (text / CLOSE reason / not checked), the body's
//           tile count (tiles of UTF8_TILE bytes of the 16-B aligned address space that holds the
//           body), the unfinished tail from the body's last three bytes, the exclusive scan of
//           the tile counts inside its block of 256 slots and the block's sum;
//   scan    one block: exclusive scan of the block sums, the total;
//   tiles   a fixed grid; every wave takes an equal, contiguous share of the tiles, finds the
//           slot of a tile by a 64-ary search (ballot) over the block sums and the block's 256
//           offsets, and keeps it while its tiles stay inside that message. A tile is 4 rows of
//           64 x 16-B nontemporal loads at natural alignment; the head and tail bytes of a body
//           are masked to 0. A lane looks back at the previous lane's last three bytes (the
//           previous row's lane 63, or one extra dword load at a tile's edge; the carried bytes
//           at a body's first byte). A chunk of ASCII bytes after nothing unfinished costs one
//           OR-reduce; any other chunk walks its 16 bytes through the rule. A byte in error
//           sets one bit of the slot's record (a vector atomic OR, at most one per wave and tile);
//   finish  one thread per slot: verdict, first_bad (atomic min), and the last listed message
//           writes the segment's state word.
// Every output is written with plain stores or vector atomics.
#include "../../include/wsframe_amd_text.h"
#include "ws_scan.h"
#include "ws_utf8.h"

#define UTF8_T 256                       // threads per block, and slots per plan block
#define UTF8_ROWS 4                      // rows of 64 chunks per tile
#define UTF8_TILE_CHUNKS (64 * UTF8_ROWS)
#define UTF8_TILE (16 * UTF8_TILE_CHUNKS)  // 4096 bytes
#define UTF8_WAVES_PER_CU 32             // tile grid: 8 blocks of 4 waves per CU

// slot record: bits 0-25 the state word's tail (n, bytes), 27 a byte in error, 28-29 class,
// 30 hopeless (continued after FAILED), 31 open
#define UTF8_I_ERR (1u << 27)
#define UTF8_I_TEXT (1u << 28)
#define UTF8_I_CLOSE (2u << 28)
#define UTF8_I_HOPELESS (1u << 30)
#define UTF8_I_OPEN (1u << 31)

struct Utf8Body {
    u64 addr;        // address of the first checked byte
    u64 len;         // checked bytes
    u32 carry3;      // the three bytes before it (p3 | p2 << 8 | p1 << 16), 0 = none
    u32 info;        // class bits (0: not checked)
};

// Class and checked range of message `m` of segment s (its slot record's class bits).
__device__ __forceinline__ Utf8Body utf8_body(const unsigned char* out, const WebsocketFrameDesc_t* desc,
                                              const WebsocketMsgDesc_t& m, const u32* state, u32 s, u32 max_frames) {
    Utf8Body b;
    b.addr = reinterpret_cast<uintptr_t>(out) + m.out_off;
    b.len = m.len;
    b.carry3 = 0;
    b.info = m.complete ? 0u : UTF8_I_OPEN;
    if (m.continued) {
        const u32 st = state ? state[s] : 0u;
        if (st & WS_UTF8_ST_PENDING) {
            b.info |= UTF8_I_TEXT;
            if (st & WS_UTF8_ST_FAILED) b.info |= UTF8_I_HOPELESS;
            b.carry3 = ws_utf8_state_last3(st);
        }
        return b;
    }
    const u32 type = m.first_frame < max_frames ? desc[(u64)s * max_frames + m.first_frame].type : 0xFFu;
    if (type == WEBSOCKET_TEXT_FRAME) {
        b.info |= UTF8_I_TEXT;
    } else if (type == WEBSOCKET_CLOSE_FRAME && m.complete == 1 && m.n_frames == 1) {
        b.info |= UTF8_I_CLOSE;                       // the reason: body bytes [2, len)
        b.addr += b.len < 2 ? b.len : 2;
        b.len -= b.len < 2 ? b.len : 2;
    }
    return b;
}

__device__ __forceinline__ u32 utf8_tiles(const Utf8Body& b) {
    if (!(b.info & (UTF8_I_TEXT | UTF8_I_CLOSE)) || (b.info & UTF8_I_HOPELESS) || b.len == 0) return 0;
    return (u32)(((b.addr & 15) + b.len + (UTF8_TILE - 1)) / UTF8_TILE);
}

__global__ __launch_bounds__(UTF8_T) void ws_utf8_plan(const unsigned char* out, const WebsocketFrameDesc_t* desc,
                                                       const WebsocketMsgDesc_t* msg, const u32* nmsg, u32 nseg,
                                                       u32 max_frames, const u32* state, u32* first_bad, u32* info,
                                                       u32* loff, u32* blocksum, u32* segflag) {
    __shared__ u32 wsum[UTF8_T / 64];
    const u64 slot = (u64)blockIdx.x * UTF8_T + threadIdx.x;
    const u64 nslots = (u64)nseg * max_frames;
    u32 tiles = 0;
    if (slot < nslots) {
        const u32 s = (u32)(slot / max_frames), i = (u32)(slot - (u64)s * max_frames);
        if (i == 0 && first_bad) first_bad[s] = WEBSOCKET_TEXT_NONE;
        u32 inf = 0;
        if (i < nmsg[s]) {
            const WebsocketMsgDesc_t m = msg[slot];
            if (m.continued) atomicOr(&segflag[s], 1u);
            const Utf8Body b = utf8_body(out, desc, m, state, s, max_frames);
            inf = b.info;
            if (inf & (UTF8_I_TEXT | UTF8_I_CLOSE)) {
                tiles = utf8_tiles(b);
                // the last three bytes of the bytes so far: the carry, then the body
                u32 last3 = b.carry3;
                if (!(inf & UTF8_I_HOPELESS) && b.len) {
                    const gu8* p = gptr<unsigned char>(reinterpret_cast<const void*>(b.addr));
                    if (b.len >= 3) last3 = p[b.len - 3] | (u32)p[b.len - 2] << 8 | (u32)p[b.len - 1] << 16;
                    else if (b.len == 2) last3 = (last3 >> 16) | (u32)p[0] << 8 | (u32)p[1] << 16;
                    else last3 = (last3 >> 8) | (u32)p[0] << 16;
                }
                const u32 n = ws_utf8_tail_len((last3 >> 16) & 0xFFu, (last3 >> 8) & 0xFFu, last3 & 0xFFu);
                inf |= ws_utf8_state_pack(n, last3) & 0x03FFFFFFu;
            }
        }
        info[slot] = inf;
    }
    // exclusive scan of the block's tile counts
    u32 excl;
    const u32 total = ws_block_sum<UTF8_T>(tiles, wsum, &excl);
    loff[slot] = excl;                                // (loff and info are padded to whole blocks)
    if (threadIdx.x == 0) blocksum[blockIdx.x] = total;
}

// exclusive scan of the nb block sums in place; bo[nb] and head[0] take the total
__global__ __launch_bounds__(1024) void ws_utf8_scan(u32* bo, u32 nb, u32* head) {
    __shared__ u32 part[1024];
    ws_offsets_scan(bo, nb, head, part);
}

__global__ __launch_bounds__(UTF8_T) void ws_utf8_tiles(const unsigned char* out, const WebsocketFrameDesc_t* desc,
                                                        const WebsocketMsgDesc_t* msg, u32 max_frames, const u32* state,
                                                        const u32* head, const u32* bo, u32 nb, u32* info,
                                                        const u32* loff) {
    const u32 lane = threadIdx.x & 63;
    const u32 wave = blockIdx.x * (UTF8_T / 64) + (threadIdx.x >> 6), nw = gridDim.x * (UTF8_T / 64);
    const u32 total = head[0];
    const u32 per = (u32)(((u64)total + nw - 1) / nw);
    const u64 t0 = (u64)wave * per;
    const u64 t1 = t0 + per < total ? t0 + per : total;
    u64 slot = 0, slot_lo = 0, slot_hi = 0;             // the slot of the current tile and its tile range
    u64 a0 = 0, nchunks = 0, bend = 0;
    u32 ph = 0, carry3 = 0;
    for (u64 t = t0; t < t1; ++t) {
        if (t >= slot_hi) {
            // the last block, then the last slot of it, that starts at or before tile t
            const u32 b = ws_wave_search([&](u32 i) { return bo[i]; }, nb, (u32)t, lane);
            const u32 bbase = bo[b];
            const u32* const lb = loff + (u64)b * UTF8_T;
            const u32 j = ws_wave_search([&](u32 i) { return lb[i]; }, UTF8_T, (u32)t - bbase, lane);
            slot = (u64)b * UTF8_T + j;
            const Utf8Body bd = utf8_body(out, desc, msg[slot], state, (u32)(slot / max_frames), max_frames);
            slot_lo = (u64)bbase + loff[slot];
            slot_hi = slot_lo + utf8_tiles(bd);
            ph = (u32)(bd.addr & 15);
            a0 = bd.addr - ph;
            bend = ph + bd.len;                         // the body's end, from a0
            nchunks = (bend + 15) / 16;
            carry3 = bd.carry3;
            if (t >= slot_hi) return;                   // (cannot happen: the plan counted these tiles)
        }
        const u64 c0 = (t - slot_lo) * UTF8_TILE_CHUNKS;
        const gu32x4* const base = gptr<u32x4>(reinterpret_cast<const void*>(a0));
        u32x4 v[UTF8_ROWS];
#pragma unroll
        for (int u = 0; u < UTF8_ROWS; ++u) {
            const u64 c = c0 + (u64)u * 64 + lane;
            v[u] = u32x4{0, 0, 0, 0};
            if (c < nchunks) v[u] = ld16<1>(base + c);
        }
        // the three bytes before the tile: the last dword of the chunk before it (a whole chunk
        // of this body: the body's first chunk is the first chunk of tile 0)
        u32 edge3 = 0;
        if (c0 != 0 && lane == 0) edge3 = *(reinterpret_cast<const gu32*>(base + c0) - 1) >> 8;
        bool bad = false;
#pragma unroll
        for (int u = 0; u < UTF8_ROWS; ++u) {
            const u64 cw = c0 + (u64)u * 64;            // wave-uniform
            if (cw >= nchunks) break;
            const u64 c = cw + lane;
            u32 cover = 0;
            if (c < nchunks) {
                const u32 lo = c == 0 ? ph : 0u;
                const u64 rem = bend - 16 * c;
                const u32 hi = rem >= 16 ? 16u : (u32)rem;
                cover = (0xFFFFu >> (16 - hi)) & (0xFFFFu << lo) & 0xFFFFu;
            }
            if (cover != 0xFFFFu && c < nchunks) {      // a body's head or tail chunk: bytes outside it read as 0
                v[u].x &= nib_to_bytemask(cover & 15u);
                v[u].y &= nib_to_bytemask((cover >> 4) & 15u);
                v[u].z &= nib_to_bytemask((cover >> 8) & 15u);
                v[u].w &= nib_to_bytemask(cover >> 12);
            }
            u32 own3 = 0;
            if (c == 0 && carry3) {
                // the carried bytes stand just before the body's first byte: chunk bytes
                // ph-3 .. ph-1, those before the chunk in this lane's own look-back
                const int sh = (int)ph - 3;
                u64 l64 = 0, h64 = 0;
                if (sh <= 0) l64 = carry3 >> (8 * -sh);
                else if (sh < 8) { l64 = (u64)carry3 << (8 * sh); h64 = sh > 5 ? (u64)carry3 >> (8 * (8 - sh)) : 0; }
                else h64 = (u64)carry3 << (8 * (sh - 8));
                v[u].x |= (u32)l64; v[u].y |= (u32)(l64 >> 32); v[u].z |= (u32)h64; v[u].w |= (u32)(h64 >> 32);
                own3 = ph < 3 ? (carry3 << (8 * ph)) & 0xFFFFFFu : 0u;
            }
            u32 last3 = ws_utf8_chunk_last3((u32)__shfl_up((int)v[u].w, 1));
            if (u > 0) {
                const u32 row3 = ws_utf8_chunk_last3((u32)__shfl((int)v[u - 1].w, 63));
                if (lane == 0) last3 = row3;
            } else if (lane == 0) {
                last3 = edge3;
            }
            if (c == 0) last3 = own3;
            if (!ws_utf8_chunk_plain(v[u].x, v[u].y, v[u].z, v[u].w, last3))
                bad |= (ws_utf8_chunk_err(v[u].x, v[u].y, v[u].z, v[u].w, last3) & cover) != 0;
        }
        if (__ballot(bad) && lane == 0) atomicOr(&info[slot], UTF8_I_ERR);
    }
}

__global__ __launch_bounds__(UTF8_T) void ws_utf8_finish(const u32* nmsg, u32 nseg, u32 max_frames, const u32* info,
                                                         const u32* segflag, u32* state, u32* verdict, u32* first_bad) {
    const u64 slot = (u64)blockIdx.x * UTF8_T + threadIdx.x;
    if (slot >= (u64)nseg * max_frames) return;
    const u32 s = (u32)(slot / max_frames), i = (u32)(slot - (u64)s * max_frames);
    const u32 n = nmsg[s];
    if (i >= n) return;
    const u32 inf = info[slot];
    const bool checked = (inf & (UTF8_I_TEXT | UTF8_I_CLOSE)) != 0, open = (inf & UTF8_I_OPEN) != 0;
    // a complete message must leave nothing unfinished; an open one only needs no byte in error
    const bool bad = checked && ((inf & (UTF8_I_HOPELESS | UTF8_I_ERR)) || (!open && ws_utf8_state_n(inf)));
    verdict[slot] = !checked ? WEBSOCKET_TEXT_NA : (bad ? WEBSOCKET_TEXT_INVALID : WEBSOCKET_TEXT_VALID);
    if (bad && first_bad) atomicMin(&first_bad[s], i);
    if (i == n - 1 && state) {
        if (open) state[s] = !(inf & UTF8_I_TEXT) ? 0u : (bad ? WS_UTF8_ST_PENDING | WS_UTF8_ST_FAILED
                                                              : WS_UTF8_ST_PENDING | (inf & 0x03FFFFFFu));
        else if (segflag[s]) state[s] = 0u;           // a continued message closed the pending one
    }
}

extern "C" WSFRAME_AMD_TEXT_EXPORT int websocketframeBatchValidateTextDevice(
    const unsigned char* d_out, const WebsocketFrameDesc_t* d_desc, const WebsocketMsgDesc_t* d_msg,
    const unsigned int* d_nmsg, unsigned int nseg, unsigned int max_frames, unsigned int* d_text_state,
    unsigned int* d_verdict, unsigned int* d_first_bad, void* hip_stream) {
    if (nseg == 0) return 0;
    if (!d_out || !d_desc || !d_msg || !d_nmsg || !d_verdict || max_frames == 0)
        return ws_set_msg("websocketframeBatchValidateTextDevice: invalid argument");
    if ((reinterpret_cast<uintptr_t>(d_desc) | reinterpret_cast<uintptr_t>(d_msg)) & 7)
        return ws_set_msg("websocketframeBatchValidateTextDevice: d_desc/d_msg not 8-B aligned");
    const u64 nslots = (u64)nseg * max_frames;
    if (nslots > (1ull << 30)) return ws_set_msg("websocketframeBatchValidateTextDevice: nseg * max_frames > 2^30");
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    const u32 nb = (u32)((nslots + UTF8_T - 1) / UTF8_T);
    // workspace (u32 words): head[4], block offsets[nb + 1], slot records, slot offsets, segment flags
    const size_t bo_off = 4, info_off = (bo_off + nb + 1 + 3) & ~(size_t)3, loff_off = info_off + (size_t)nb * UTF8_T,
                 flag_off = loff_off + (size_t)nb * UTF8_T, words = flag_off + nseg;
    WsSlot slot;
    int rc = slot.acquire(st);
    if (rc) return rc;
    void* p = nullptr;
    if ((rc = slot.buffer(WS_BUF_TEXT, words * sizeof(u32), 0, &p))) return rc;
    u32* const ws = reinterpret_cast<u32*>(p);
    hipError_t e = hipMemsetAsync(ws + flag_off, 0, (size_t)nseg * sizeof(u32), st);
    if (e != hipSuccess) return ws_set_err("websocketframeBatchValidateTextDevice: memset", e);
    hipLaunchKernelGGL(ws_utf8_plan, dim3(nb), dim3(UTF8_T), 0, st, d_out, d_desc, d_msg, d_nmsg, nseg, max_frames,
                       d_text_state, d_first_bad, ws + info_off, ws + loff_off, ws + bo_off, ws + flag_off);
    hipLaunchKernelGGL(ws_utf8_scan, dim3(1), dim3(1024), 0, st, ws + bo_off, nb, ws);
    hipLaunchKernelGGL(ws_utf8_tiles, dim3((u32)slot.cus * (UTF8_WAVES_PER_CU / (UTF8_T / 64))), dim3(UTF8_T), 0, st, d_out,
                       d_desc, d_msg, max_frames, d_text_state, ws, ws + bo_off, nb, ws + info_off, ws + loff_off);
    hipLaunchKernelGGL(ws_utf8_finish, dim3(nb), dim3(UTF8_T), 0, st, d_nmsg, nseg, max_frames, ws + info_off,
                       ws + flag_off, d_text_state, d_verdict, d_first_bad);
    e = hipGetLastError();
    return e == hipSuccess ? 0 : ws_set_err("websocketframeBatchValidateTextDevice launch", e);
}
