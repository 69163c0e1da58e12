// stage_clock.hpp — wall-clock per stage of a voxelPS run (`voxelPS --timing <file.json>`: VERDICT r04 item 4 -- the Gauss-Newton iterations are
// milliseconds, the decode / fusion / dump stages around them are what a user waits for).  Scopes nest: a stage's time includes the stages opened inside it.
#pragma once
#include <chrono>
#include <fstream>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

namespace psgsdf_host {

struct StageClock {
    std::vector<std::pair<std::string, double>> acc; std::vector<long long> calls; std::mutex mu;      // (the background writer thread books its stages too)
    size_t slot(const std::string& n) { std::lock_guard<std::mutex> g(mu); for (size_t i = 0; i < acc.size(); ++i) if (acc[i].first == n) return i; acc.emplace_back(n, 0.0); calls.push_back(0); return acc.size() - 1; }
    struct Scope {
        StageClock& c; size_t i; std::chrono::steady_clock::time_point t0;
        Scope(StageClock& c_, const std::string& n) : c(c_), i(c_.slot(n)), t0(std::chrono::steady_clock::now()) {}
        ~Scope() { const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); std::lock_guard<std::mutex> g(c.mu); c.acc[i].second += dt; c.calls[i] += 1; }
    };
    static StageClock& get() { static StageClock c; return c; }
    double of(const std::string& n) { return acc[slot(n)].second; }
    bool write_json(const std::string& path, const std::string& extra = "") {
        std::ofstream f(path.c_str()); if (!f.is_open()) return false;
        f << "{\"stages_s\": {";
        for (size_t i = 0; i < acc.size(); ++i) f << (i ? ", " : "") << "\"" << acc[i].first << "\": " << acc[i].second;
        f << "}, \"calls\": {";
        for (size_t i = 0; i < acc.size(); ++i) f << (i ? ", " : "") << "\"" << acc[i].first << "\": " << calls[i];
        f << "}" << extra << "}\n";
        return true;
    }
};
#define PSG_STAGE_CAT2(a, b) a##b
#define PSG_STAGE_CAT(a, b) PSG_STAGE_CAT2(a, b)
#define PSG_STAGE(name) ::psgsdf_host::StageClock::Scope PSG_STAGE_CAT(psg_stage_, __LINE__)(::psgsdf_host::StageClock::get(), name)

}  // namespace psgsdf_host
