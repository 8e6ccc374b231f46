// io_tables.h -- what the device-side I/O engines (engine_ingest.cpp, engine_egress.cpp) share, host C++: a table row decoded
// by a copy, the tables a launch searches, their launches format by format, and the device form's upload-launch-wait.  A call
// form supplies its row, the job of a row and the launch of one format's jobs.
#pragma once
#include <cstring>
#include <string>
#include <vector>

#include "internal.h"

namespace fvad {

inline size_t up16(size_t b) { return (b + 15) / 16 * 16; }

// Row: a struct of uint64_t fields that restates a table layout of fvad.h field for field (a static_assert on its size stands
// where it is defined), so that a row is decoded by a copy
template <typename Row>
Row row(const uint64_t* rows, size_t i)
{
    Row r;
    memcpy(&r, rows + i * (sizeof(Row) / 8), sizeof(Row));
    return r;
}

// The tables of one call or batch: per file format (a launch decodes or encodes one) the jobs and their unit prefix, laid out
// in ONE blob whose parts start on 16-byte boundaries, so that one copy carries them to the device.
struct Tables {
    struct Set { size_t o_jobs = 0, o_prefix = 0; uint32_t n_jobs = 0, n_units = 0; } set[3];
    std::vector<char> blob;
};

// A launch is one workgroup of 256 lanes per unit; HIP runtimes refuse a grid of 2^32 threads or more, so a launch takes fewer
// than 2^24 units (about 270 GB of file bytes: the ring never gets near it, a device form only with a buffer of HBM's size).
constexpr uint64_t kMaxUnits = (1ull << 24) - 1;

// one format's jobs and the units in front of each (`prefix` gets its last entry here) appended to the blob
template <typename Job>
void pack(const std::vector<Job>& jobs, std::vector<uint32_t>& prefix, uint64_t units, Tables::Set& set, std::vector<char>& blob)
{
    set.n_jobs = (uint32_t)jobs.size();
    set.n_units = (uint32_t)units;
    if (jobs.empty()) return;
    prefix.push_back((uint32_t)units);
    set.o_jobs = blob.size();
    set.o_prefix = set.o_jobs + up16(jobs.size() * sizeof(Job));
    blob.resize(set.o_prefix + up16(prefix.size() * 4));
    memcpy(blob.data() + set.o_jobs, jobs.data(), jobs.size() * sizeof(Job));
    memcpy(blob.data() + set.o_prefix, prefix.data(), prefix.size() * 4);
}

// make(row, job) fills the job of a row and returns its units; a row of 0 units writes nothing and gets no job.  false: more
// than kMaxUnits units in one launch.
template <typename Job, typename Row, typename Make>
bool build_tables(const std::vector<Row>& rows, Make make, Tables& t)
{
    t.blob.clear();
    for (int f = 0; f < 3; ++f) {
        std::vector<Job> jobs;
        std::vector<uint32_t> prefix;
        uint64_t units = 0;
        for (const Row& s : rows) {
            if ((int)s.format != f) continue;
            Job j{};
            const uint64_t n = make(s, j);
            if (n == 0) continue;
            if (n > kMaxUnits) return false;
            prefix.push_back((uint32_t)units);
            jobs.push_back(j);
            units += n;
            if (units > kMaxUnits) return false;
        }
        pack(jobs, prefix, units, t.set[f], t.blob);
    }
    return true;
}

// the launches of one set of tables, in the order of the formats (queued on ctx->stream): one(f, set) launches a format's jobs
template <typename One>
int launch_tables(const Tables& t, One one)
{
    for (int f = 0; f < 3; ++f) {
        if (!t.set[f].n_units) continue;
        const int rc = one(f, t.set[f]);
        if (rc != FVAD_OK) return rc;
    }
    return FVAD_OK;
}

// The device form behind its refusals: the tables of all rows, then one allocation for the tap table (if the form has one)
// and the tables, the copies, launch(t, d_blob, d_table) and the wait.  `too_many` ends the refusal of more than 2^24 tiles
// ("write in batches"), `what` names the allocation in its error.
template <typename Row, typename Job, typename Make, typename Launch>
int device_form(fvad_ctx* ctx, const std::string& who, const char* too_many, const char* what, const uint64_t* rows, size_t n_rows,
                const std::vector<float>& table, Make make, Launch launch)
{
    std::vector<Row> all(n_rows);
    for (size_t i = 0; i < n_rows; ++i) all[i] = row<Row>(rows, i);
    Tables t;
    if (!build_tables<Job>(all, make, t)) return set_err(ctx, FVAD_ERR_INVALID_ARGUMENT, who + ": more than 2^24 tiles in one call: " + too_many);
    if (t.blob.empty()) return FVAD_OK; // nothing to write
    const size_t o_blob = up16(table.size() * 4);
    hipSetDevice(ctx->device);
    char* d = nullptr; // the tap table, then the row tables
    if (hipMalloc((void**)&d, o_blob + t.blob.size()) != hipSuccess) { (void)hipGetLastError(); return set_err(ctx, FVAD_ERR_ALLOC_FAILED, who + ": hipMalloc of the " + what + " failed"); }
    auto run = [&]() -> int {
        if (!table.empty()) FVAD_HIP(ctx, hipMemcpyAsync(d, table.data(), table.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        FVAD_HIP(ctx, hipMemcpyAsync(d + o_blob, t.blob.data(), t.blob.size(), hipMemcpyHostToDevice, ctx->stream));
        const int rc = launch(t, d + o_blob, reinterpret_cast<const float*>(d));
        if (rc != FVAD_OK) return rc;
        FVAD_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return FVAD_OK;
    };
    const int rc = run();
    if (rc != FVAD_OK) (void)hipStreamSynchronize(ctx->stream);
    hipFree(d);
    return rc;
}

} // namespace fvad
