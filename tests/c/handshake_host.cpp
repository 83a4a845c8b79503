// Host driver of util_amd/csrc/ws_handshake.h (tests/test_handshake_host.py): the handshake's rule
// compiled by a host compiler. As a shared object it exposes ws_hs_one to ctypes; with
// -DHS_HOST_MAIN it is a program of its own (the form a sanitizer build takes) that reads cases
// from a text file, one per line:
//     <request hex or -> <ret> <key_off> <key_len> <proto_off> <proto_len> <accept hex or -> <resp hex or -> <echo hex or ->
// and runs each from a heap buffer of exactly len + 32 bytes into response buffers of exactly
// resp_len bytes, so a read past the pad or a write past resp_len is an error of the sanitizer.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../util_amd/csrc/ws_handshake.h"

extern "C" void ws_hs_host_one(const unsigned char* buf, unsigned long long len, unsigned int flags,
                               WebsocketHandshakeDesc_t* hs, unsigned char* accept, unsigned char* resp,
                               unsigned int resp_cap) {
    ws_hs_one(buf, len, flags, hs, accept, resp, resp_cap);
}

// accept (28 characters) of a key alone: the SHA-1, padding and base64 part
extern "C" void ws_hs_host_accept(const unsigned char* key, unsigned int key_len, unsigned char out[32]) {
    uint32_t acc[8];
    ws_hs_accept_of(key, key_len, acc);
    for (int i = 0; i < 32; ++i) out[i] = (unsigned char)(acc[i >> 2] >> (8 * (i & 3)));
}

#ifdef HS_HOST_MAIN
static std::vector<unsigned char> unhex(const std::string& s) {
    std::vector<unsigned char> v;
    if (s == "-") return v;
    for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((unsigned char)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
    return v;
}

static int fail(size_t line, const char* what) {
    printf("handshake_host: case %zu: %s\n", line, what);
    return 1;
}

static int run_case(size_t line, const std::vector<unsigned char>& req, int ret, unsigned ko, unsigned kl, unsigned po,
                    unsigned pl, const std::vector<unsigned char>& accept, const std::vector<unsigned char>& resp,
                    unsigned flags) {
    unsigned char* buf = (unsigned char*)malloc(req.size() + 32);          // exactly len + WEBSOCKET_BATCH_PAD
    if (!req.empty()) memcpy(buf, req.data(), req.size());
    memset(buf + req.size(), 0xEE, 32);
    const size_t want = ret > 0 ? resp.size() : 0;
    unsigned char* out = (unsigned char*)malloc(want ? want : 1);          // exactly resp_len
    unsigned char acc[32];
    memset(acc, 0x5A, sizeof(acc));
    WebsocketHandshakeDesc_t d;
    ws_hs_one(buf, req.size(), flags, &d, acc, out, (unsigned)want);
    int bad = 0;
    if (d.ret != ret || d.key_off != ko || d.key_len != kl || d.proto_off != po || d.proto_len != pl || d.reserved != 0)
        bad = fail(line, "descriptor differs");
    else if (d.resp_len != want || d.flags != (ret > 0 ? WEBSOCKET_HS_RESP_WRITTEN : 0u))
        bad = fail(line, "resp_len or flags differ");
    else if (ret > 0 && (memcmp(acc, accept.data(), 28) || acc[28] || acc[29] || acc[30] || acc[31]))
        bad = fail(line, "accept differs");
    else if (ret > 0 && memcmp(out, resp.data(), want))
        bad = fail(line, "response differs");
    else if (ret <= 0 && acc[0] != 0x5A)
        bad = fail(line, "accept written without a complete request");
    if (!bad && ret > 0) {                                                  // one byte short: nothing is written
        unsigned char* small = (unsigned char*)malloc(want - 1);
        memset(small, 0x77, want - 1);
        ws_hs_one(buf, req.size(), flags, &d, nullptr, small, (unsigned)want - 1);
        if (d.flags != WEBSOCKET_HS_RESP_NO_SPACE || d.resp_len != want) bad = fail(line, "NO_SPACE not reported");
        for (size_t i = 0; i + 1 < want; ++i)
            if (small[i] != 0x77) { bad = fail(line, "written without space"); break; }
        free(small);
    }
    free(out);
    free(buf);
    return bad;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    std::vector<char> linebuf(1 << 16);
    size_t n = 0;
    int bad = 0;
    while (fgets(linebuf.data(), (int)linebuf.size(), f)) {
        std::vector<std::string> tok;
        for (char* t = strtok(linebuf.data(), " \n"); t; t = strtok(nullptr, " \n")) tok.push_back(t);
        if (tok.size() != 9) { fclose(f); return 2; }
        const std::vector<unsigned char> req = unhex(tok[0]);
        const int ret = atoi(tok[1].c_str());
        const unsigned ko = (unsigned)strtoul(tok[2].c_str(), nullptr, 10), kl = (unsigned)strtoul(tok[3].c_str(), nullptr, 10),
                       po = (unsigned)strtoul(tok[4].c_str(), nullptr, 10), pl = (unsigned)strtoul(tok[5].c_str(), nullptr, 10);
        bad |= run_case(n, req, ret, ko, kl, po, pl, unhex(tok[6]), unhex(tok[7]), 0u);
        bad |= run_case(n, req, ret, ko, kl, po, pl, unhex(tok[6]), unhex(tok[8]), WEBSOCKET_HS_ECHO_PROTOCOL);
        ++n;
    }
    fclose(f);
    if (bad || n == 0) return 1;
    printf("handshake_host ok %zu\n", n);
    return 0;
}
#endif
