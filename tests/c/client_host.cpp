// Host driver of util_amd/csrc/ws_client.h (tests/test_client_host.py): the client handshake's
// rule compiled by a host compiler. As a shared object it exposes ws_cl_verify_one and
// ws_cl_request_one to ctypes; with -DCLIENT_HOST_MAIN it is a program of its own (the form a
// sanitizer build takes) that reads cases from a text file, one per line:
//     V <response hex or -> <offered hex or -> <max_head> <ret> <reason> <status> <proto_off> <proto_len> <accept_off> <expect hex>
//     R <path hex> <proto hex or -> <host hex or -> <nonce hex> <request hex> <expect hex> <key_off>
// and runs each response from a heap buffer of exactly len + 32 bytes and each request into
// buffers of exactly req_len bytes and of one byte less, so a read past the pad or a write past
// req_len is an error of the sanitizer.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../util_amd/csrc/ws_client.h"

extern "C" void ws_cl_host_verify(const unsigned char* buf, unsigned long long len, const unsigned char* expect,
                                  const unsigned char* offered, unsigned int offered_len, unsigned int max_head,
                                  WebsocketClientVerifyDesc_t* cv) {
    ws_cl_verify_one(buf, len, expect, offered, offered_len, max_head, cv);
}

extern "C" void ws_cl_host_request(const unsigned char* path, unsigned int path_len, const unsigned char* proto,
                                   unsigned int proto_len, const unsigned char* host, unsigned int host_len,
                                   const unsigned char* nonce, unsigned char* req, unsigned int req_cap, unsigned char* expect,
                                   WebsocketClientReqDesc_t* rd) {
    ws_cl_request_one(path, path_len, proto, proto_len, host, host_len, nonce, req, req_cap, expect, rd);
}

#ifdef CLIENT_HOST_MAIN
static std::vector<unsigned char> unhex(const std::string& s) {
    std::vector<unsigned char> v;
    if (s == "-") return v;
    for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((unsigned char)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
    return v;
}

static unsigned char* heap_copy(const std::vector<unsigned char>& v, size_t extra, int fill) {
    unsigned char* p = (unsigned char*)malloc(v.size() + extra ? v.size() + extra : 1);
    if (!v.empty()) memcpy(p, v.data(), v.size());
    memset(p + v.size(), fill, extra);
    return p;
}

static int fail(size_t line, const char* what) {
    printf("client_host: case %zu: %s\n", line, what);
    return 1;
}

static unsigned num(const std::string& s) { return (unsigned)strtoul(s.c_str(), nullptr, 10); }

static int run_verify(size_t line, const std::vector<std::string>& t) {
    const std::vector<unsigned char> data = unhex(t[1]), offered = unhex(t[2]), expect = unhex(t[10]);
    unsigned char* buf = heap_copy(data, 32, 0xEE);                          // exactly len + WEBSOCKET_BATCH_PAD
    unsigned char* off = heap_copy(offered, 0, 0);                           // exactly the list
    unsigned char* exp = heap_copy(expect, 0, 0);                            // exactly 32
    WebsocketClientVerifyDesc_t d;
    ws_cl_verify_one(buf, data.size(), exp, offered.empty() ? nullptr : off, (unsigned)offered.size(), num(t[3]), &d);
    int bad = 0;
    if (d.ret != atoi(t[4].c_str()) || d.reason != num(t[5]) || d.status != num(t[6]) || d.proto_off != num(t[7]) ||
        d.proto_len != num(t[8]) || d.accept_off != num(t[9]) || d.flags != 0 || d.reserved != 0)
        bad = fail(line, "verify descriptor differs");
    free(exp);
    free(off);
    free(buf);
    return bad;
}

static int run_request(size_t line, const std::vector<std::string>& t) {
    const std::vector<unsigned char> path = unhex(t[1]), proto = unhex(t[2]), host = unhex(t[3]), nonce = unhex(t[4]),
                                     want = unhex(t[5]), expect = unhex(t[6]);
    unsigned char *p = heap_copy(path, 0, 0), *pr = heap_copy(proto, 0, 0), *h = heap_copy(host, 0, 0), *nn = heap_copy(nonce, 0, 0);
    unsigned char* out = (unsigned char*)malloc(want.size());                // exactly req_len
    unsigned char* small = (unsigned char*)malloc(want.size() - 1);          // one byte less: nothing is written
    memset(small, 0x77, want.size() - 1);
    unsigned char exp[32];
    WebsocketClientReqDesc_t d;
    int bad = 0;
    ws_cl_request_one(p, (unsigned)path.size(), pr, (unsigned)proto.size(), h, (unsigned)host.size(), nn, out,
                      (unsigned)want.size(), exp, &d);
    if (d.req_len != want.size() || d.key_off != num(t[7]) || d.flags != WEBSOCKET_CLI_REQ_WRITTEN || d.reserved != 0)
        bad = fail(line, "request descriptor differs");
    else if (memcmp(out, want.data(), want.size())) bad = fail(line, "request differs");
    else if (memcmp(exp, expect.data(), 32)) bad = fail(line, "expect differs");
    memset(exp, 0x5A, 32);
    ws_cl_request_one(p, (unsigned)path.size(), pr, (unsigned)proto.size(), h, (unsigned)host.size(), nn, small,
                      (unsigned)want.size() - 1, exp, &d);
    if (d.flags != WEBSOCKET_CLI_REQ_NO_SPACE || d.req_len != want.size()) bad = fail(line, "NO_SPACE not reported");
    if (memcmp(exp, expect.data(), 32)) bad = fail(line, "expect not written without space");
    for (size_t i = 0; i + 1 < want.size(); ++i)
        if (small[i] != 0x77) { bad = fail(line, "written without space"); break; }
    free(small);
    free(out);
    free(nn);
    free(h);
    free(pr);
    free(p);
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
        if (tok.size() == 11 && tok[0] == "V") bad |= run_verify(n, tok);
        else if (tok.size() == 8 && tok[0] == "R") bad |= run_request(n, tok);
        else { fclose(f); return 2; }
        ++n;
    }
    fclose(f);
    if (bad || n == 0) return 1;
    printf("client_host ok %zu\n", n);
    return 0;
}
#endif
