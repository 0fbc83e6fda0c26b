// trim_io.h - file plumbing of the read trimming stage's programs (oc2pm4, oc2lcr, oc2etr, oc2orderResults): whole-file record loads that refuse a
// short file, outputs that appear under their name only when they are complete (".part" + rename, as pm_job.h does), the stage's small index files.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <string>
#include <vector>

#include "trim_core.h"

namespace necat_host {
namespace trim {

inline std::string in_dir(const char* dir, const char* leaf)
{
    std::string s(dir);
    if (s.empty() || s.back() != '/') s.push_back('/');
    return s + leaf;
}

// load_num_reads, common/makedb_aux.c:58-68
inline bool load_num_reads(const char* wrk_dir, int* num_reads)
{
    const std::string p = in_dir(wrk_dir, "reads_info.txt");
    FILE* f = fopen(p.c_str(), "r");
    int nv = 0;
    const bool ok = f && fscanf(f, "%d%d", &nv, num_reads) == 2 && *num_reads >= 0;
    if (f) fclose(f);
    if (!ok) fprintf(stderr, "cannot read %s\n", p.c_str());
    return ok;
}

// make_partition_name / load_num_partitions, trim_bases/pm4_aux.c:19-50
inline std::string partition_name(const char* m4_path, int pid) { return std::string(m4_path) + ".p" + std::to_string(pid); }
inline bool load_num_partitions(const char* m4_path, int* np)
{
    const std::string p = std::string(m4_path) + ".partitions";
    FILE* f = fopen(p.c_str(), "r");
    const bool ok = f && fscanf(f, "%d", np) == 1 && *np >= 0;
    if (f) fclose(f);
    if (!ok) fprintf(stderr, "cannot read %s (run oc2pm4 first)\n", p.c_str());
    return ok;
}

// the size of a file of 96-byte records in records; false (with a line on stderr): missing, or not a whole number of records
inline bool record_count(const char* path, uint64_t* n)
{
    struct stat st;
    if (stat(path, &st) != 0 || !S_ISREG(st.st_mode)) { fprintf(stderr, "cannot open %s\n", path); return false; }
    if ((uint64_t)st.st_size % sizeof(M4)) { fprintf(stderr, "%s is truncated: %llu bytes are not a whole number of 96-byte records\n", path, (unsigned long long)st.st_size); return false; }
    *n = (uint64_t)st.st_size / sizeof(M4);
    return true;
}

inline bool load_records(const char* path, std::vector<M4>& v)
{
    uint64_t n = 0;
    if (!record_count(path, &n)) return false;
    v.resize(n);
    if (n == 0) return true;
    FILE* f = fopen(path, "rb");
    const bool ok = f && fread(v.data(), sizeof(M4), n, f) == n;
    if (f) fclose(f);
    if (!ok) fprintf(stderr, "cannot read %s\n", path);
    return ok;
}

// an output file that exists under its name only once it is complete
struct OutFile {
    FILE* f = nullptr;
    std::string path;
    bool open(const std::string& p, const char* mode)
    {
        path = p;
        f = fopen((p + ".part").c_str(), mode);
        if (!f) fprintf(stderr, "cannot write %s\n", p.c_str());
        return f != nullptr;
    }
    bool commit()
    {
        if (!f) return false;
        bool ok = !ferror(f);
        ok = fclose(f) == 0 && ok;
        f = nullptr;
        if (ok) ok = rename((path + ".part").c_str(), path.c_str()) == 0;
        if (!ok) { fprintf(stderr, "write error on %s\n", path.c_str()); unlink((path + ".part").c_str()); }
        return ok;
    }
    void discard() { if (f) { fclose(f); f = nullptr; } if (!path.empty()) unlink((path + ".part").c_str()); }
    ~OutFile() { if (f) discard(); }
};

}  // namespace trim
}  // namespace necat_host
