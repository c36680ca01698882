// probe_launch_events.hip -- what a timed kernel launch costs on its stream: N back-to-back launches of one kernel (a) with no event,
// (b) bracketed by two recorded events (hipEventRecord before and after: KernelProfile::begin / end), (c) with the pair attached to the
// dispatch (hipExtLaunchKernelGGL's startEvent / stopEvent), (d) with only a stop event attached, (e) as a profiled BPR epoch
// boundary issues them today (record, launch, three records).  Printed: microseconds per launch, host wall time over a final
// synchronisation.  The kernel is empty, or writes `words` floats (about 10 us of work) so that a packet has something to wait behind.
// Then which pairs hipEventElapsedTime accepts: start and stop of one launch; the stops of two launches; a recorded event and an
// attached stop; an attached stop and a recorded event.
// build: hipcc --offload-arch=gfx950 -O3 scripts/probe_launch_events.hip -o build/probe_launch_events
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <chrono>
#include <cstdio>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

__global__ void k_work(float* p, int words) {
    const int stride = gridDim.x * blockDim.x;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < words; i += stride) p[i] = (float)i;
}

int main() {
    const int N = 2000, kWords = 1 << 24;
    float* buf;
    CK(hipMalloc(&buf, (size_t)kWords * 4));
    hipStream_t st;
    CK(hipStreamCreate(&st));
    std::vector<hipEvent_t> ev((size_t)4 * N);
    for (auto& e : ev) CK(hipEventCreate(&e));
    const char* names[5] = {"no event", "recorded pair", "attached pair", "attached stop only", "record + launch + 3 records"};
    for (int words : {0, kWords}) {
        const dim3 grid(words ? 2048 : 1), block(256);
        printf("kernel: %s\n", words ? "writes 64 MB" : "empty");
        for (int mode = 0; mode < 5; mode++) {
            double best = 1e30;
            for (int rep = 0; rep < 3; rep++) {
                CK(hipStreamSynchronize(st));
                const auto t0 = std::chrono::steady_clock::now();
                for (int i = 0; i < N; i++) {
                    hipEvent_t *e = &ev[(size_t)4 * i];
                    switch (mode) {
                    case 0: hipLaunchKernelGGL(k_work, grid, block, 0, st, buf, words); break;
                    case 1:
                        (void)hipEventRecord(e[0], st);
                        hipLaunchKernelGGL(k_work, grid, block, 0, st, buf, words);
                        (void)hipEventRecord(e[1], st);
                        break;
                    case 2: hipExtLaunchKernelGGL(k_work, grid, block, 0, st, e[0], e[1], 0, buf, words); break;
                    case 3: hipExtLaunchKernelGGL(k_work, grid, block, 0, st, nullptr, e[1], 0, buf, words); break;
                    case 4:
                        (void)hipEventRecord(e[0], st);
                        hipLaunchKernelGGL(k_work, grid, block, 0, st, buf, words);
                        (void)hipEventRecord(e[1], st);
                        (void)hipEventRecord(e[2], st);
                        (void)hipEventRecord(e[3], st);
                        break;
                    }
                }
                CK(hipGetLastError());
                CK(hipStreamSynchronize(st));
                const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / N;
                if (us < best) best = us;
            }
            printf("  %-28s %8.2f us per launch (best of 3 x %d)", names[mode], best, N);
            if (mode >= 1) {  // the kernel's own span as the events give it, mean over the last repetition
                double sum = 0;
                int ok = 0;
                for (int i = 0; i < N; i++) {
                    float ms = 0;
                    hipEvent_t a = mode == 3 ? (i ? ev[(size_t)4 * (i - 1) + 1] : nullptr) : ev[(size_t)4 * i], b = ev[(size_t)4 * i + 1];
                    if (a && hipEventElapsedTime(&ms, a, b) == hipSuccess) sum += ms, ok++;
                }
                (void)hipGetLastError();
                printf("   span %s: %8.2f us mean of %d", mode == 3 ? "stop to stop" : "start to stop", ok ? sum / ok * 1e3 : 0.0, ok);
            }
            printf("\n");
        }
    }
    // ---- which pairs hipEventElapsedTime accepts ----
    const dim3 grid(2048), block(256);
    hipEvent_t s1 = ev[0], p1 = ev[1], s2 = ev[2], p2 = ev[3], r0 = ev[4], r1 = ev[5];
    CK(hipEventRecord(r0, st));
    hipExtLaunchKernelGGL(k_work, grid, block, 0, st, s1, p1, 0, buf, kWords);
    hipExtLaunchKernelGGL(k_work, grid, block, 0, st, s2, p2, 0, buf, kWords);
    CK(hipEventRecord(r1, st));
    CK(hipGetLastError());
    // a second stream waits on an attached stop, as the preparation stream would on a consumed chunk
    hipStream_t st2;
    CK(hipStreamCreate(&st2));
    const hipError_t w = hipStreamWaitEvent(st2, p2, 0);
    printf("hipStreamWaitEvent on an attached stop: %s\n", hipGetErrorString(w));
    hipLaunchKernelGGL(k_work, dim3(1), block, 0, st2, buf, 0);
    CK(hipStreamSynchronize(st2));
    printf("hipEventQuery of that stop after the waiting stream drained: %s\n", hipGetErrorString(hipEventQuery(p2)));
    CK(hipStreamSynchronize(st));
    struct { const char* what; hipEvent_t a, b; } combos[] = {
        {"start and stop of one launch", s1, p1},     {"stops of two launches", p1, p2},
        {"start of one, stop of the next", s1, p2},   {"recorded event, attached stop", r0, p1},
        {"attached stop, recorded event", p2, r1},    {"attached start, recorded event", s1, r1},
        {"recorded pair around both", r0, r1},
    };
    for (auto& c : combos) {
        float ms = -1;
        const hipError_t e = hipEventElapsedTime(&ms, c.a, c.b);
        (void)hipGetLastError();
        printf("hipEventElapsedTime(%-32s): %-24s %9.2f us\n", c.what, hipGetErrorString(e), ms * 1e3);
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(st2);
    (void)hipStreamDestroy(st);
    (void)hipFree(buf);
    return 0;
}
