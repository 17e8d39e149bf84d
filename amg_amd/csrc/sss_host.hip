// sss_host.hip — process infrastructure of the engine (declared in sss_engine.hpp): the HIP error
// report, the host worker pool behind parallel_chunks, and the host -> device copy.  No kernel.
#include "sss_engine.hpp"

#include <algorithm>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <sched.h>
#include <sys/resource.h>
#include <sys/syscall.h>
#include <unistd.h>

namespace sss {

int hip_fail(hipError_t e, const char *what, const char *file, int line)
{
    fprintf(stderr, "### ERROR: HIP call %s failed at %s:%d: %s\n", what, file, line, hipGetErrorString(e));
    return ERROR_MISC;
}

// ---- host worker pool (sss_engine.hpp) ----------------------------------------------------------
// Threads: SSS_HOST_THREADS, else the usable CPUs (affinity mask, capped by a cgroup v2 cpu.max
// quota), at most 32.
static int usable_cpus()
{
    const char *e = getenv("SSS_HOST_THREADS");
    if (e && *e) return std::max(1, atoi(e));
    int n = (int)std::max(1u, std::thread::hardware_concurrency());
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof(set), &set) == 0) n = std::max(1, CPU_COUNT(&set));
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[32] = {0};
        long long period = 0;
        if (fscanf(f, "%31s %lld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0)
            n = std::min(n, (int)std::max(1LL, (atoll(q) + period - 1) / period));
        fclose(f);
    }
    return std::min(n, 32);
}

// Upload helpers run at a lower CPU priority (nice SSS_HOST_NICE, default 10): when the mirror is
// built while the setup runs (sss_hip_setup_create), the setup's serial RS pass and its OpenMP
// regions keep their cores and the upload takes what they leave idle.
void host_thread_background()
{
    const char *e = getenv("SSS_HOST_NICE");
    const int nice = (e && *e) ? atoi(e) : 10;
    if (nice > 0) (void)setpriority(PRIO_PROCESS, (id_t)syscall(SYS_gettid), nice);
}

namespace {
// Several callers may hold jobs at once (the mirror's level tasks run side by side after the setup):
// each job is a loop body that returns once its shared chunk counter is exhausted; an idle worker
// joins any open job, and a job closes for newcomers as soon as one of its threads has returned.
struct HostPool {
    struct Job {
        const std::function<void()> *work = nullptr;
        int inside = 0;
        bool open = false;
    };
    static constexpr int kJobs = 8;
    std::mutex mu;
    std::condition_variable cv, done_cv;
    Job jobs[kJobs];
    int nt = 1, rr = 0;
    static thread_local bool in_worker;
    HostPool()
    {
        nt = usable_cpus();
        for (int t = 1; t < nt; ++t) std::thread([this] { loop(); }).detach();   // lives as long as the process
    }
    int open_job() const
    {
        for (int k = 0; k < kJobs; ++k)
            if (jobs[(rr + k) % kJobs].open) return (rr + k) % kJobs;
        return -1;
    }
    void loop()
    {
        in_worker = true;
        host_thread_background();
        for (;;) {
            int j;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return open_job() >= 0; });
                j = open_job();
                rr = (j + 1) % kJobs;
                ++jobs[j].inside;
            }
            (*jobs[j].work)();
            std::lock_guard<std::mutex> lk(mu);
            jobs[j].open = false;   // its counter is exhausted: nothing left to join
            if (--jobs[j].inside == 0) done_cv.notify_all();
        }
    }
    bool run(const std::function<void()> &work)
    {
        if (in_worker) return false;
        int j = -1;
        {
            std::lock_guard<std::mutex> lk(mu);
            for (int k = 0; k < kJobs && j < 0; ++k)
                if (!jobs[k].work) j = k;
            if (j < 0) return false;
            jobs[j].work = &work;
            jobs[j].inside = 0;
            jobs[j].open = true;
        }
        cv.notify_all();
        work();
        {
            std::unique_lock<std::mutex> lk(mu);
            jobs[j].open = false;
            done_cv.wait(lk, [&] { return jobs[j].inside == 0; });
            jobs[j].work = nullptr;
        }
        return true;
    }
};
thread_local bool HostPool::in_worker = false;

HostPool &host_pool()
{
    static HostPool *p = new HostPool();   // never destroyed: detached workers outlive static teardown
    return *p;
}
}   // namespace

int host_pool_threads() { return host_pool().nt; }
bool host_pool_run(const std::function<void()> &work) { return host_pool().run(work); }

// Host -> device copy of a large host array through a ring of pinned staging buffers: host threads
// copy chunk k + 1 into one buffer while the DMA engine moves chunk k out of another (a pageable
// hipMemcpy of the 400^3 hierarchy's ~60 GB ran at ~3 GB/s).  Small copies go straight through.
int h2d(void *dst, const void *src, size_t bytes)
{
    constexpr size_t kChunk = (size_t)32 << 20;
    constexpr int kSlots = 4;
    if (bytes < ((size_t)4 << 20)) {
        if (bytes) SSS_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
        return 0;
    }
    static std::mutex mu;
    static char *buf[kSlots];
    static hipEvent_t ev[kSlots];
    static hipStream_t st = nullptr;
    std::lock_guard<std::mutex> guard(mu);
    if (!st) {
        for (int k = 0; k < kSlots; ++k) {
            SSS_HIP(hipHostMalloc((void **)&buf[k], kChunk));
            SSS_HIP(hipEventCreateWithFlags(&ev[k], hipEventDisableTiming));
        }
        SSS_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    }
    const char *s = static_cast<const char *>(src);
    char *d = static_cast<char *>(dst);
    int slot = 0;
    for (size_t off = 0; off < bytes; off += kChunk, slot = (slot + 1) % kSlots) {
        const size_t n = std::min(kChunk, bytes - off);
        SSS_HIP(hipEventSynchronize(ev[slot]));   // the slot's previous DMA has finished
        const int parts = 8;
        const size_t per = (n + parts - 1) / parts;
        parallel_chunks(parts, 1, [&](int a, int e) {
            for (int t = a; t < e; ++t) {
                const size_t lo = (size_t)t * per, hi = std::min(n, lo + per);
                if (lo < hi) std::memcpy(buf[slot] + lo, s + off + lo, hi - lo);
            }
        });
        SSS_HIP(hipMemcpyAsync(d + off, buf[slot], n, hipMemcpyHostToDevice, st));
        SSS_HIP(hipEventRecord(ev[slot], st));
    }
    SSS_HIP(hipStreamSynchronize(st));
    return 0;
}

}  // namespace sss
