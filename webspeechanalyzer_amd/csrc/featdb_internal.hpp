// featdb_internal.hpp — the device feature DB (specification FD-1) as featdb.hip owns it and as its consumers read it:
// train.hip (wsa_trainer_create_db) and dbstats.hip (wsa_featdb_dbstats_create).  Internal to csrc/.
#pragma once
#include <string>
#include "host_plan.hpp"

namespace wsa_fd {

// a device table that grows on demand and is never shrunk (the scratch of append, gather and ranges); not part of a DevArena, which only frees at the end
template <typename T>
struct Grow {
    T* p = nullptr; size_t cap = 0;
    Grow() = default;
    Grow(const Grow&) = delete;
    Grow& operator=(const Grow&) = delete;
    ~Grow() { if (p) (void)hipFree(p); }
    bool ensure(size_t n) {
        if (n <= cap && p) return true;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }                    // (hipFree waits for the work that may still read it)
        void* q = nullptr;
        if (hipMalloc(&q, (n ? n : 1) * sizeof(T)) != hipSuccess) return false;
        p = reinterpret_cast<T*>(q); cap = n ? n : 1;
        return true;
    }
};

}  // namespace wsa_fd

struct wsa_featdb {
    wsa_ctx* ctx = nullptr;
    int width = 0;                                       // 53, 264 or 23
    uint32_t capacity = 0, count = 0;                    // rows allocated, rows held
    double* d_feat = nullptr;                            // [capacity][width], rows 0 .. count - 1 valid
    uint32_t *h_total = nullptr, *d_total = nullptr;     // mapped pinned word: the rows the keep kernel kept
    wsa_fd::Grow<uint32_t> kept;                         // source row of every kept row, in source order
    wsa_fd::Grow<uint32_t> rows;                         // a row list on the device (gather, ranges)
    wsa_fd::Grow<uint64_t> part;                         // ranges: per chunk and column {min key, max key, NaN seen}, then the result
    uint32_t* h_rows = nullptr; size_t h_rows_cap = 0;   // pinned staging of a row list
    hipEvent_t ev_rows = nullptr;                        // the copy that last read h_rows
    wsa::DevArena mem;
    // FD-2: the stream set whose steps append to this DB (wsa_stream_set_featdb), and whether one of its steps has been launched whose
    // outcome the host has not read yet — `count` is then behind the device, and whatever reads or moves it is refused
    const void* attached_to = nullptr;
    bool step_pending = false;
};

namespace wsa_fd {

// which rows are kept: all (levels 5 / 13: no kernel decides that), the level-12 rule, the last utterance row per clip / stream
enum { FD_ALL = 0, FD_L12 = 1, FD_L11 = 2 };
// the level that goes with a width: the mode of the keep rule, or -1 (levels 3, 4 and 10 store nothing)
inline int mode_for(int level, int width) {
    if ((level == 5 || level == 13) && width == WSA_NFEAT) return FD_ALL;
    if (level == 12 && width == 23) return FD_L12;
    if (level == 11 && width == WSA_NUTT) return FD_L11;
    return -1;
}

// "" or why `what` is refused on this DB right now (FD-2 "who owns the count")
inline std::string pending_refusal(const wsa_featdb* db, const char* what) {
    if (!db->step_pending) return "";
    return std::string(what) + ": a stream step that appends to this feature DB (" + std::to_string(db->count) + " rows before it) has not been collected yet: "
           "call wsa_stream_collect first";
}

// "" or why a row list over the DB is refused: the first entry outside its rows
inline std::string rows_refusal(const wsa_featdb* db, const uint32_t* rows, uint32_t n) {
    for (uint32_t i = 0; i < n; i++)
        if (rows[i] >= db->count)
            return "rows[" + std::to_string(i) + "] = " + std::to_string(rows[i]) + " is outside the DB's " + std::to_string(db->count) + " rows";
    return "";
}

}  // namespace wsa_fd
