// seq_reader.h - FASTA / FASTQ records, plain or gzip, with klib's kseq semantics (klib/kseq.h): the reader of oc2mkdb, shared with the read
// trimming stage's programs (oc2etr, oc2orderResults), which must cut names and sequences exactly where the reference's kseq_read cuts them.
#pragma once
#include <ctype.h>
#include <zlib.h>

#include <string>
#include <vector>

namespace necat_host {

// byte-stream reader with the buffer discipline of klib's kstream (16 KB blocks over gzread)
struct Stream {
    gzFile f = nullptr;
    std::vector<unsigned char> buf = std::vector<unsigned char>(16384);
    int begin = 0, end = 0;
    bool eof = false, err = false;
    int getc()
    {
        if (err) return -3;
        if (begin >= end) {
            if (eof) return -1;
            begin = 0;
            end = gzread(f, buf.data(), (unsigned)buf.size());
            if (end == 0) { eof = true; return -1; }
            if (end < 0) { eof = true; err = true; end = 0; return -3; }
        }
        return buf[begin++];
    }
    // ks_getuntil2 (klib/kseq.h:92-145): append bytes up to the delimiter (a line end, or any white space when
    // `space`), consume the delimiter, report it in *dret; < 0 when nothing could be read
    int until(bool space, std::string& s, int* dret, bool append)
    {
        bool gotany = false;
        if (dret) *dret = 0;
        if (!append) s.clear();
        for (;;) {
            if (err) return -3;
            if (begin >= end) {
                if (eof) break;
                begin = 0;
                end = gzread(f, buf.data(), (unsigned)buf.size());
                if (end == 0) { eof = true; break; }
                if (end < 0) { eof = true; err = true; end = 0; return -3; }
            }
            int i = begin;
            if (space) { while (i < end && !isspace(buf[i])) ++i; }
            else { while (i < end && buf[i] != '\n') ++i; }
            gotany = true;
            s.append((const char*)buf.data() + begin, (size_t)(i - begin));
            begin = i + 1;
            if (i < end) { if (dret) *dret = buf[i]; break; }
        }
        if (!gotany && eof && begin >= end) return -1;
        if (!space && s.size() > 1 && s.back() == '\r') s.pop_back();
        return (int)s.size();
    }
};

// kseq_read (klib/kseq.h:178-218): >= 0 sequence length, -1 end of file, -2 truncated quality string
struct Reader {
    Stream ks;
    int last_char = 0;
    std::string name, comment, seq, qual;
    int next()
    {
        int c;
        if (last_char == 0) {
            while ((c = ks.getc()) >= 0 && c != '>' && c != '@') {}
            if (c < 0) return c;
            last_char = c;
        }
        comment.clear(); seq.clear(); qual.clear();
        int r = ks.until(true, name, &c, false);
        if (r < 0) return r;
        if (c != '\n') ks.until(false, comment, nullptr, false);
        while ((c = ks.getc()) >= 0 && c != '>' && c != '+' && c != '@') {
            if (c == '\n') continue;
            seq.push_back((char)c);
            ks.until(false, seq, nullptr, true);
        }
        if (c == '>' || c == '@') last_char = c;
        if (c != '+') return (int)seq.size();
        while ((c = ks.getc()) >= 0 && c != '\n') {}
        if (c == -1) return -2;
        while (ks.until(false, qual, nullptr, true) >= 0 && qual.size() < seq.size()) {}
        last_char = 0;
        if (seq.size() != qual.size()) return -2;
        return (int)seq.size();
    }
};

}  // namespace necat_host
