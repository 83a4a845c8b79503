/* tools/exp_reply.py's host side: websocketframeControlRepliesHost looped over the segments of a
 * batch by `nthreads` threads, each a contiguous range of segments, each segment's reply at the
 * offset a first pass computed (tx_capacity 0: lengths only), as a host path would pack them.
 * Returns the total reply length, or -1. */
#include <pthread.h>
#include <stdlib.h>

#include "../include/wsframe_amd_reply.h"

typedef struct Job {
    const unsigned char* buf;
    const unsigned long long* seg_off;
    const WebsocketFrameDesc_t* desc;
    const WebsocketSegResult_t* res;
    unsigned int max_frames, flags, lo, hi;
    unsigned char* tx;
    unsigned long long* tx_off; /* pass 0: lengths; pass 1: offsets */
    WebsocketReplyResult_t* out;
    int pass;
    long long bad;
} Job;

static void* work(void* p) {
    Job* j = (Job*)p;
    for (unsigned int s = j->lo; s < j->hi; ++s) {
        const long long n = websocketframeControlRepliesHost(
            j->buf, j->seg_off[s], j->desc + (size_t)s * j->max_frames, j->res + s, j->max_frames, j->flags, 0, 0, 0, 0,
            j->pass ? j->tx + j->tx_off[s] : 0, j->pass ? ~0ULL : 0, j->out + s);
        if (n < 0) j->bad = 1;
        if (!j->pass) j->tx_off[s] = (unsigned long long)n;
    }
    return 0;
}

long long reply_host_loop(const unsigned char* buf, const unsigned long long* seg_off, const WebsocketFrameDesc_t* desc,
                          const WebsocketSegResult_t* res, unsigned int nseg, unsigned int max_frames, unsigned int flags,
                          unsigned char* tx, unsigned long long* tx_off, WebsocketReplyResult_t* out, int nthreads) {
    if (nthreads < 1 || nthreads > 64) return -1;
    pthread_t th[64];
    Job job[64];
    unsigned long long total = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int t = 0; t < nthreads; ++t) {
            const Job j = {buf, seg_off, desc, res, max_frames, flags, (unsigned int)((unsigned long long)nseg * t / nthreads),
                           (unsigned int)((unsigned long long)nseg * (t + 1) / nthreads), tx, tx_off, out, pass, 0};
            job[t] = j;
            if (pthread_create(&th[t], 0, work, &job[t])) return -1;
        }
        for (int t = 0; t < nthreads; ++t) {
            pthread_join(th[t], 0);
            if (job[t].bad) return -1;
        }
        if (!pass) {                                  /* lengths -> exclusive offsets */
            for (unsigned int s = 0; s < nseg; ++s) {
                const unsigned long long n = tx_off[s];
                tx_off[s] = total;
                total += n;
            }
            tx_off[nseg] = total;
        }
    }
    return (long long)total;
}
