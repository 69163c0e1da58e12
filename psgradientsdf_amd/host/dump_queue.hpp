// dump_queue.hpp — where the dump files are written: one background thread per process, so that the optimisation goes on while a dump is being
// formatted, and, in a run on N devices, every rank's piece of the one file at its place.
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <fcntl.h>
#include <functional>
#include <iostream>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unistd.h>
#include <vector>

#include "../../include/psgsdf.h"
#include "stage_clock.hpp"
#include "text_format.hpp"

namespace psgsdf_host {

// One background thread that formats and writes the dumps in the order they were issued; drain() before anything that must see the files.
class DumpQueue {
    std::thread th_; std::mutex m_; std::condition_variable cv_, idle_; std::deque<std::function<void()>> q_; bool stop_ = false, busy_ = false;
    void run() {
        for (;;) {
            std::function<void()> job;
            { std::unique_lock<std::mutex> l(m_); cv_.wait(l, [&] { return stop_ || !q_.empty(); }); if (q_.empty()) return; job = std::move(q_.front()); q_.pop_front(); busy_ = true; }
            { PSG_STAGE("background: format + write the dump files"); job(); }
            { std::lock_guard<std::mutex> l(m_); busy_ = false; }
            idle_.notify_all();
        }
    }
    std::atomic<int> failures_{0};
public:
    static DumpQueue& get() { static DumpQueue q; return q; }
    void report_failure() { failures_.fetch_add(1); }      // a job could not open / write its file: surfaced by failures() after drain() (voxelPS exits non-zero)
    int failures() const { return failures_.load(); }
    void push(std::function<void()> job) {
        std::lock_guard<std::mutex> l(m_);
        if (!th_.joinable()) th_ = std::thread([this] { run(); });
        q_.push_back(std::move(job)); cv_.notify_one();
    }
    void drain() { PSG_STAGE("wait for the background writer"); std::unique_lock<std::mutex> l(m_); idle_.wait(l, [&] { return q_.empty() && !busy_; }); }
    ~DumpQueue() { { std::lock_guard<std::mutex> l(m_); stop_ = true; } cv_.notify_all(); if (th_.joinable()) th_.join(); }
};

// ---- one run on N devices (`voxelPS --gpus N`: one process per GPU, the volume cut into z-slabs; no reference counterpart) ---------------------------
// main() fills this in before anything else.  Every rank runs the same program on the same inputs (decodes the frames, selects the keyframes); the
// engine calls are collective.  Rank 0 narrates and writes the small text files; the big ones are written by ALL ranks: each formats the lines of
// its share (psgsdf_extract_* on a multi-rank context) and writes them into their place in the one file -- the places come from an exclusive scan of
// the byte counts over the ranks (psgsdf_comm_allreduce_host).  The files are the single-process files line for line, up to what the slabs'
// rank-order sums do to the last digit of a value.
struct RankInfo { int rank = 0, n = 1, device = 0; bool sockets = false; std::vector<int> fds; std::vector<uint8_t> id; };
inline RankInfo& rank_info() { static RankInfo r; return r; }
inline bool multi_rank() { return rank_info().n > 1; }
inline bool lead_rank() { return rank_info().rank == 0; }
// k numbers of every rank -> the sums over the ranks in front of this one, and over all
// `local_ok` = false: this rank failed in front of the collective.  It STILL enters it (a rank that returned early left the others blocked in the
// all-reduce: ADVICE r05) and its flag travels as one more summed element, so that every rank returns false together.
inline bool scan_over_ranks(psgsdf_ctx* ctx, const std::vector<double>& mine, std::vector<double>& before, std::vector<double>& total, bool local_ok = true) {
    const RankInfo& ri = rank_info(); const size_t k = mine.size(), k1 = k + 1;
    std::vector<double> all(k1 * (size_t)ri.n, 0.0);
    for (size_t i = 0; i < k; ++i) all[k1 * (size_t)ri.rank + i] = local_ok ? mine[i] : 0.0;
    all[k1 * (size_t)ri.rank + k] = local_ok ? 0.0 : 1.0;
    if (psgsdf_comm_allreduce_host(ctx, all.data(), (int)all.size())) return false;
    before.assign(k, 0.0); total.assign(k, 0.0);
    double failed = 0.0;
    for (int r = 0; r < ri.n; ++r) { for (size_t i = 0; i < k; ++i) { if (r < ri.rank) before[i] += all[k1 * (size_t)r + i]; total[i] += all[k1 * (size_t)r + i]; } failed += all[k1 * (size_t)r + k]; }
    return failed == 0.0;
}
inline size_t bytes_of(const std::vector<TextOut>& parts) { size_t b = 0; for (auto& p : parts) b += p.s.size(); return b; }
struct FilePiece { long long offset; std::shared_ptr<std::vector<TextOut>> parts; };
// this rank's pieces of a file all ranks write: rank 0 also owns the header and the file's final length
inline void write_shared_file(const std::string& file, const std::string& header, long long total_bytes, std::vector<FilePiece> pieces) {
    DumpQueue::get().push([=] {
        const int fd = open(file.c_str(), O_CREAT | O_WRONLY, 0644);      // (no O_TRUNC: the other ranks write their pieces into the same file at the same time; the lead rank sets the final length)
        if (fd < 0) { std::cerr << "couldn't open " << file << std::endl; DumpQueue::get().report_failure(); return; }
        auto put = [&](const char* p, size_t n, long long at) { while (n) { const ssize_t k = pwrite(fd, p, n, (off_t)at); if (k <= 0) { std::cerr << "couldn't write " << file << std::endl; return false; } p += k; n -= (size_t)k; at += k; } return true; };
        bool ok = true;
        if (lead_rank()) ok = put(header.data(), header.size(), 0) && ftruncate(fd, (off_t)total_bytes) == 0;
        for (auto& pc : pieces) { long long at = pc.offset; for (auto& t : *pc.parts) { if (ok && !t.s.empty()) ok = put(t.s.data(), t.s.size(), at); at += (long long)t.s.size(); } }
        if (close(fd) != 0) ok = false;
        if (!ok) DumpQueue::get().report_failure();      // (this rank's piece is missing from a file the other ranks completed: the run reports it, voxelps_main.cpp)
    });
}

}  // namespace psgsdf_host
