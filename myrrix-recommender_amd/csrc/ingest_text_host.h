// ingest_text_host.h -- host side of the text half of the ingest path (mals_ingest_append_text / _read_file /
// _read_dir, include/myrrix_als.h).  Host code of ingest_api.hip.  Expects before it: ingest_host.h (the ingest object, the
// launch helpers, scan_u32, grow_records) and ingest_text_kernels.h.
//
// The host does what java.io does for the reference -- list the directory (InputFilesReader.java:71-86), open and
// inflate files (FileLineIterator.java:92-102), hand the bytes on in blocks -- and keeps the two counters whose
// meaning is sequential (IFR:92-98: lines, badLines).  Splitting into lines, parsing every line and compacting the
// records happen on the device (ingest_text_kernels.h, text_parse.h).  A block boundary inside a line is healed by
// carrying the unterminated tail (device to device) in front of the next block.
#pragma once

#include <dirent.h>
#include <sys/stat.h>
#include <zlib.h>

namespace {

constexpr size_t TEXT_PAD = 128;  // readable bytes behind the text (16-byte and 8-byte aligned window loads)

// room for `want` elements, by at least half the capacity at a time; the first `used` elements are kept
template <typename T>
int reserve_text(mals_ingest g, DeviceBuffer<T>& b, size_t want, size_t used = 0) {
  if (want > b.capacity()) ICHK(g, b.grow_keep(std::max(want, b.capacity() + b.capacity() / 2), used, g->stream));
  return MALS_OK;
}

int text_fail(mals_ingest g, int code, const std::string& msg) {
  g->text_failed = true;
  g->text_fail_code = code;
  g->text_fail_msg = msg;
  return fail(g, code, msg);
}

int ensure_record_capacity(mals_ingest g, int64_t extra) {
  const int64_t cap = record_capacity(g);
  if (g->n + extra <= cap) return MALS_OK;
  return grow_records(g, std::max<int64_t>(g->n + extra, cap + cap / 2));
}

// One block: the bytes d_text[0, total) are on the device; lines are taken from [0, region) (region ends right after
// a line terminator, or at `total` for the last block of a file).
int process_text_region(mals_ingest g, size_t region) {
  if (region == 0) return MALS_OK;
  if (region >= 0xffffff00ull) return fail(g, MALS_INVALID_ARG, "text block too large");
  // HIP-event time of the kernels only: allocations (which cost milliseconds to seconds, depending on the box) sit
  // between the timed segments
  EventPair ev;
  ICHK(g, ev.ensure());
  const hipEvent_t e0 = ev.begin, e1 = ev.end;
  auto seg_end = [&]() -> int {
    ICHK(g, hipEventRecord(e1, g->stream));
    ICHK(g, hipEventSynchronize(e1));
    float ms = 0.f;
    ICHK(g, hipEventElapsedTime(&ms, e0, e1));
    g->parse_ms += ms;
    return MALS_OK;
  };
  ICHK(g, hipEventRecord(e0, g->stream));
  // 1. line starts
  const int64_t n_blk = ((int64_t)region + LT_BLOCK_BYTES - 1) / LT_BLOCK_BYTES;
  const int64_t tiles = (n_blk + SC_TILE - 1) / SC_TILE;
  if (int rc = reserve_text(g, g->t_block_counts, (size_t)n_blk)) return rc;
  if (int rc = reserve_text(g, g->t_tile_sums, (size_t)tiles + 2)) return rc;
  Scratch s;
  s.tile_sums = g->t_tile_sums.get();
  s.total = g->t_tile_sums.get() + tiles;  // one word behind the tile sums
  ITRY(launch_grid(g, {(unsigned)n_blk}, line_count_kernel, g->d_text.get(), (int64_t)region, g->t_block_counts.get()));
  unsigned n_lines = 0;
  if (int rc = scan_u32(g, s, g->t_block_counts.get(), g->t_block_counts.get(), n_blk, &n_lines)) return rc;
  if (int rc = seg_end()) return rc;
  if (n_lines == 0) return fail(g, MALS_HIP_ERROR, "internal: a non-empty text region without a line");
  // sequential rule IFR:96-98: the line that follows the 101st bad line throws
  if (g->abort_armed) return text_fail(g, MALS_IO_ERROR, "Too many bad lines; aborting");
  // 2. per-line arrays
  const size_t L = n_lines;
  if (L > g->t_starts.capacity()) {
    g->t_starts.reset(); g->t_status.reset(); g->t_user.reset(); g->t_item.reset(); g->t_value.reset();
    g->t_flag.reset(); g->t_defer.reset();
    const size_t cap = L + L / 4;
    ICHK(g, g->t_status.alloc(cap + 8));
    ICHK(g, g->t_user.alloc(cap));
    ICHK(g, g->t_item.alloc(cap));
    ICHK(g, g->t_value.alloc(cap));
    ICHK(g, g->t_flag.alloc(cap));
    ICHK(g, g->t_defer.alloc(cap));
    ICHK(g, g->t_starts.alloc(cap));  // last: its capacity says that all of them exist
  }
  {
    const int64_t lt = ((int64_t)L + SC_TILE - 1) / SC_TILE;
    if (int rc = reserve_text(g, g->t_tile_sums, (size_t)std::max(lt, tiles) + 2)) return rc;
    s.tile_sums = g->t_tile_sums.get();
    s.total = g->t_tile_sums.get() + std::max(lt, tiles);
  }
  if (!g->t_counters) ICHK(g, g->t_counters.alloc(sizeof(TextCounters) + 3 * sizeof(unsigned)));   // (+ the tag cursors and the empty-tag line)
  TextCounters* counters = reinterpret_cast<TextCounters*>(g->t_counters.get());
  ICHK(g, hipEventRecord(e0, g->stream));
  ICHK(g, hipMemsetAsync(counters, 0, sizeof(TextCounters) + 3 * sizeof(unsigned), g->stream));
  ITRY(launch_grid(g, {(unsigned)n_blk}, line_starts_kernel, g->d_text.get(), (int64_t)region, g->t_block_counts.get(), g->t_starts.get()));
  const unsigned lgrid = (unsigned)((L + 255) / 256);
  const int first = g->lines == 0 ? 1 : 0;
  // 3. parse: the bulk, then whatever it handed on
  ITRY(launch_grid(g, {lgrid}, parse_lines_kernel, g->d_text.get(), g->t_starts.get(), (int64_t)L, (unsigned)region, first, g->t_status.get(), g->t_user.get(),
                   g->t_item.get(), g->t_value.get(), g->t_defer.get(), counters));
  ITRY(launch_grid(g, {(unsigned)std::min<size_t>((L + 63) / 64, 4096), 64}, parse_deferred_kernel, g->d_text.get(), g->t_starts.get(), (int64_t)L, (unsigned)region,
                   first, g->t_status.get(), g->t_user.get(), g->t_item.get(), g->t_value.get(), g->t_defer.get(), counters));
  const int64_t ct = ((int64_t)L + CT_TILE - 1) / CT_TILE;  // t_flag: records per tile, then their exclusive scan
  ITRY(launch_grid(g, {(unsigned)ct}, line_summary_kernel, g->t_status.get(), (int64_t)L, g->t_flag.get(), counters));
  unsigned n_records = 0;
  ITRY(scan_u32(g, s, g->t_flag.get(), g->t_flag.get(), ct, nullptr));
  ICHK(g, hipMemcpyAsync(&n_records, s.total, sizeof(unsigned), hipMemcpyDeviceToHost, g->stream));
  TextCounters c;
  ICHK(g, hipMemcpyAsync(&c, counters, sizeof(c), hipMemcpyDeviceToHost, g->stream));
  if (int rc = seg_end()) return rc;
  c.records = n_records;
  // 4. the sequential part of the contract
  //    (the line numbers of the first 101 bad lines are kept: a group finish places the abort in the whole stream.  Any ingest
  //    may be share 0 of a group, so every one keeps them: one copy of the block's status bytes to the host per block with a
  //    bad line, until 101 bad lines are seen -- at most 101 copies of L bytes per ingest)
  const bool want_pos = c.bad && g->bad_pos.size() < 101;
  if (c.fatal || g->bad_lines + (int64_t)c.bad > 100 || want_pos) {
    std::vector<uint8_t> st(L);
    ICHK(g, hipMemcpy(st.data(), g->t_status.get(), L, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < L && g->bad_pos.size() < 101; ++i)
      if ((st[i] & 15) == text::ST_BAD) g->bad_pos.push_back(g->lines + (int64_t)i + 1);
    int64_t bad = g->bad_lines;
    for (size_t i = 0; i < L && (c.fatal || g->bad_lines + (int64_t)c.bad > 100); ++i) {
      if (bad > 100) return text_fail(g, MALS_IO_ERROR, "Too many bad lines; aborting");
      const int k = st[i] & 15;
      if (k == text::ST_FATAL) {
        g->fatal_line = g->lines + (int64_t)i + 1;
        return text_fail(g, MALS_INVALID_ARG,
                         "line " + std::to_string(g->lines + (int64_t)i + 1) +
                             ": a token that is a lone '\"' (the reference throws StringIndexOutOfBoundsException here)");
      }
      if (k == text::ST_BAD) ++bad;
    }
  }
  // MALS_INGEST_OPT_LIVE_TAGS: a line that sets the empty tag throws out of ServerRecommender.ingest; here the text fails
  if (g->live_tags && (c.user_tags || c.item_tags)) {
    unsigned* first_empty = reinterpret_cast<unsigned*>(counters + 1) + 2;
    unsigned got = 0;
    ITRY(launch(g, (int64_t)L, empty_tag_set_kernel, g->t_status.get(), g->t_value.get(), (int64_t)L, first_empty));
    ICHK(g, hipMemcpyAsync(&got, first_empty, sizeof(unsigned), hipMemcpyDeviceToHost, g->stream));
    ICHK(g, hipStreamSynchronize(g->stream));
    if (got)
      return text_fail(g, MALS_INVALID_ARG,
                       "line " + std::to_string(g->lines + (int64_t)(0xffffffffu - got) + 1) +
                           ": a line that sets the empty tag (the reference's setUserTag / setItemTag throw IllegalArgumentException here)");
  }
  if (g->finished) g->free_results();   // any accepted text (also lines that yield no record) makes the last finish stale
  g->bad_lines += c.bad;
  g->abort_armed = g->bad_lines > 100;
  g->lines += (int64_t)L;
  g->header_lines += c.header;
  g->skipped_lines += c.skipped;
  g->slow_lines += c.deferred;
  // 5. records, in file order
  if (c.records) {
    if (g->n + (int64_t)c.records >= MALS_INGEST_MAX_RECORDS) return text_fail(g, MALS_INVALID_ARG, "at most 2^36 records per ingest");
    if (int rc = ensure_record_capacity(g, c.records)) return rc;
    ICHK(g, hipEventRecord(e0, g->stream));
    ITRY(launch_grid(g, {(unsigned)ct}, compact_records_kernel, g->t_status.get(), g->t_flag.get(), (int64_t)L, g->t_user.get(), g->t_item.get(), g->t_value.get(),
                     g->d_user.get() + g->n, g->d_item.get() + g->n, g->d_value.get() + g->n, g->live_tags ? g->d_kind.get() + g->n : nullptr));
    ITRY(seg_end());
    g->n += c.records;
  }
  if (c.user_tags || c.item_tags) {
    if (int rc = reserve_text(g, g->d_tags[0], g->n_tags_raw[0] + c.user_tags, g->n_tags_raw[0])) return rc;
    if (int rc = reserve_text(g, g->d_tags[1], g->n_tags_raw[1] + c.item_tags, g->n_tags_raw[1])) return rc;
    unsigned* cursors = reinterpret_cast<unsigned*>(counters + 1);
    ITRY(launch(g, (int64_t)L, collect_tags_kernel, g->t_status.get(), (int64_t)L, g->t_user.get(), g->t_item.get(), g->d_tags[0].get() + g->n_tags_raw[0],
                g->d_tags[1].get() + g->n_tags_raw[1], cursors));
    g->n_tags_raw[0] += c.user_tags;
    g->n_tags_raw[1] += c.item_tags;
  }
  g->text_bytes += (int64_t)region;
  return MALS_OK;
}

// position just behind the last line terminator of bytes[0, m) that can be recognised without looking past m
size_t last_terminator_end(const uint8_t* b, size_t m) {
  for (size_t q = m; q-- > 0;) {
    if (b[q] == '\n') return q + 1;
    if (b[q] == '\r' && q + 1 < m) return q + 1;
  }
  return 0;
}

int append_text_impl(mals_ingest g, const uint8_t* bytes, int64_t n_bytes, int mem_kind, bool eof) {
  const size_t block = g->text_block_bytes;
  int64_t off = 0;
  bool first_pass = true;
  while (off < n_bytes || (first_pass && eof && g->carry_len > 0)) {
    first_pass = false;
    const size_t m = (size_t)std::min<int64_t>(n_bytes - off, (int64_t)block);
    const bool last = eof && off + (int64_t)m == n_bytes;
    const size_t total = g->carry_len + m;
    if (total + TEXT_PAD > g->d_text.capacity()) ICHK(g, g->d_text.alloc(((std::max(total, block) + TEXT_PAD + 4095) / 4096) * 4096));
    ICHK(g, g->t_ev.ensure());
    ICHK(g, hipEventRecord(g->t_ev.begin, g->stream));
    if (g->carry_len) ICHK(g, hipMemcpyAsync(g->d_text.get(), g->d_carry.get(), g->carry_len, hipMemcpyDeviceToDevice, g->stream));
    if (m)
      ICHK(g, hipMemcpyAsync(g->d_text.get() + g->carry_len, bytes + off, m, mem_kind == MALS_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice,
                             g->stream));
    ICHK(g, hipMemsetAsync(g->d_text.get() + total, 0, TEXT_PAD, g->stream));
    // (the carried tail was translated with its own block: translating it again changes nothing)
    if (g->tab_delimiter && total) ITRY(launch(g, (int64_t)total, text_tabs_to_commas_kernel, g->d_text.get(), (int64_t)total));
    ICHK(g, hipEventRecord(g->t_ev.end, g->stream));
    // where the complete lines end
    size_t region;
    uint8_t last_byte = 0;
    if (last) {
      region = total;
    } else {
      size_t cut = 0;  // within the new bytes
      if (mem_kind == MALS_MEM_HOST) {
        cut = last_terminator_end(bytes + off, m);
        if (m) last_byte = bytes[off + (int64_t)m - 1];
      } else {
        std::vector<uint8_t> tail;
        size_t look = std::min<size_t>(m, 1 << 16);
        for (;;) {
          tail.resize(look);
          ICHK(g, hipMemcpy(tail.data(), bytes + off + (int64_t)(m - look), look, hipMemcpyDeviceToHost));
          const size_t c = last_terminator_end(tail.data(), look);
          if (c || look == m) {
            cut = c ? (m - look) + c : 0;
            break;
          }
          look = std::min<size_t>(m, look * 16);
        }
        if (m) last_byte = tail[look - 1];
      }
      if (cut) region = g->carry_len + cut;
      else region = (g->carry_ends_cr && m) ? g->carry_len : 0;  // the carried '\r' turned out to be a terminator of its own
    }
    if (int rc = process_text_region(g, region)) return rc;
    {
      float ms = 0.f;
      ICHK(g, hipEventSynchronize(g->t_ev.end));
      ICHK(g, hipEventElapsedTime(&ms, g->t_ev.begin, g->t_ev.end));
      g->stage_ms += ms;  // bringing the block in front of the kernels: PCIe for host bytes, a device copy otherwise
    }
    // the tail waits for the next block
    const size_t rest = total - region;
    if (rest) {
      if (rest > g->d_carry.capacity()) ICHK(g, g->d_carry.alloc(rest + rest / 2 + 4096));
      ICHK(g, hipMemcpyAsync(g->d_carry.get(), g->d_text.get() + region, rest, hipMemcpyDeviceToDevice, g->stream));
    }
    ICHK(g, hipStreamSynchronize(g->stream));
    g->carry_len = rest;
    if (m) g->carry_ends_cr = rest > 0 && last_byte == '\r';
    else if (!rest) g->carry_ends_cr = false;
    off += (int64_t)m;
  }
  if (eof) {
    g->carry_len = 0;
    g->carry_ends_cr = false;
  }
  return MALS_OK;
}

bool ends_with(const std::string& s, const char* suf) {
  const size_t n = strlen(suf);
  return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

// PatternFilenameFilter(".+\\.csv(\\.(zip|gz))?")  (IFR:71)
bool is_input_file_name(const std::string& name) {
  std::string stem = name;
  if (ends_with(stem, ".zip")) stem.resize(stem.size() - 4);
  else if (ends_with(stem, ".gz")) stem.resize(stem.size() - 3);
  return ends_with(stem, ".csv") && stem.size() > 4;
}

}  // namespace

extern "C" {

int mals_ingest_set_option(mals_ingest g, int32_t option, int64_t value) {
  if (!g) return MALS_INVALID_ARG;
  if (g->spent) return fail(g, MALS_INVALID_ARG, "the ingest's records went into mals_group_ingest_finish: create a new ingest");
  switch (option) {
    case MALS_INGEST_OPT_KNOWN_ITEMS:
      g->want_known = value != 0;
      return MALS_OK;
    case MALS_INGEST_OPT_RESERVE_RECORDS: {
      if (value < 0 || value >= MALS_INGEST_MAX_RECORDS) return fail(g, MALS_INVALID_ARG, "at most 2^36 records per ingest");
      ICHK(g, hipSetDevice(g->device));
      return ensure_record_capacity(g, std::max<int64_t>(0, value - g->n));
    }
    case MALS_INGEST_OPT_PARTITION_RECORDS:
      if (value != 0 && (value < 64 || value > MALS_INGEST_ONE_SHOT_MAX)) return fail(g, MALS_INVALID_ARG, "partition records: 0 (default) or 64 .. 2^31 - 256");
      g->part_cap = value;
      return MALS_OK;
    case MALS_INGEST_OPT_SHARE:
      if (value < 0 || value >= MALS_SPLIT_MAX_SHARES) return fail(g, MALS_INVALID_ARG, "share: 0 .. 255");
      if (g->n || g->lines || g->text_bytes || g->carry_len) return fail(g, MALS_INVALID_ARG, "the share is set before the first append");
      g->share = (int32_t)value;
      return MALS_OK;
    case MALS_INGEST_OPT_TAB_DELIMITER:
      g->tab_delimiter = value != 0;
      return MALS_OK;
    case MALS_INGEST_OPT_LIVE_TAGS:
      if (g->n || g->lines || g->text_bytes || g->carry_len) return fail(g, MALS_INVALID_ARG, "live tags are chosen before the first append");
      g->live_tags = value != 0;
      g->d_kind.reset();
      if (g->live_tags && record_capacity(g) > 0) {   // (MALS_INGEST_OPT_RESERVE_RECORDS came first)
        ICHK(g, hipSetDevice(g->device));
        ICHK(g, g->d_kind.alloc((size_t)record_capacity(g)));
      }
      return MALS_OK;
    case MALS_INGEST_OPT_TEXT_BLOCK_BYTES:
      if (value < 1 || value > (int64_t)1 << 31) return fail(g, MALS_INVALID_ARG, "text block: 1 byte .. 2 GiB");
      g->text_block_bytes = (size_t)value;
      return MALS_OK;
    default:
      return fail(g, MALS_INVALID_ARG, "unknown ingest option");
  }
}

int mals_ingest_append_text(mals_ingest g, const void* bytes, int64_t n_bytes, int mem_kind, int32_t end_of_file) {
  if (!g) return MALS_INVALID_ARG;
  if (g->spent) return fail(g, MALS_INVALID_ARG, "the ingest's records went into mals_group_ingest_finish: create a new ingest");
  if (g->text_failed) return fail(g, g->text_fail_code, g->text_fail_msg);
  if (n_bytes < 0 || (n_bytes > 0 && !bytes)) return fail(g, MALS_INVALID_ARG, "bad text block");
  if (mem_kind != MALS_MEM_HOST && mem_kind != MALS_MEM_DEVICE) return fail(g, MALS_INVALID_ARG, "mem_kind must be MALS_MEM_HOST or MALS_MEM_DEVICE");
  ICHK(g, hipSetDevice(g->device));
  return append_text_impl(g, static_cast<const uint8_t*>(bytes), n_bytes, mem_kind, end_of_file != 0);
}

int mals_ingest_read_file(mals_ingest g, const char* path) {
  if (!g || !path) return MALS_INVALID_ARG;
  if (g->spent) return fail(g, MALS_INVALID_ARG, "the ingest's records went into mals_group_ingest_finish: create a new ingest");
  if (g->text_failed) return fail(g, g->text_fail_code, g->text_fail_msg);
  ICHK(g, hipSetDevice(g->device));
  const std::string p(path);
  if (ends_with(p, ".zip")) {
    // FileLineIterator.java:98-99 wraps the file in a ZipInputStream and never calls getNextEntry(): such a stream reads
    // as empty, so the reference takes no line from a .zip input.  The file must still exist (FileInputStream).
    FILE* f = fopen(path, "rb");
    if (!f) return text_fail(g, MALS_IO_ERROR, std::string("cannot open ") + path);
    fclose(f);
    return append_text_impl(g, nullptr, 0, MALS_MEM_HOST, true);
  }
  const size_t buf_bytes = std::min<size_t>(g->text_block_bytes, (size_t)64 << 20);
  if (buf_bytes > g->h_pinned.capacity()) ICHK(g, g->h_pinned.alloc(buf_bytes));
  uint8_t* buf = g->h_pinned.get();
  if (ends_with(p, ".gz")) {
    gzFile f = gzopen(path, "rb");
    if (!f) return text_fail(g, MALS_IO_ERROR, std::string("cannot open ") + path);
    (void)gzbuffer(f, 1 << 20);
    bool any = false;
    for (;;) {
      const int got = gzread(f, buf, (unsigned)std::min<size_t>(buf_bytes, 1u << 30));
      if (got < 0 || (!any && gzdirect(f))) {  // GZIPInputStream: "Not in GZIP format" / corrupt member -> IOException
        gzclose(f);
        return text_fail(g, MALS_IO_ERROR, std::string("not a readable gzip file: ") + path);
      }
      any = true;
      const bool eof = got == 0 || gzeof(f);
      if (int rc = append_text_impl(g, buf, got, MALS_MEM_HOST, eof)) {
        gzclose(f);
        return rc;
      }
      if (eof) break;
    }
    gzclose(f);
    return MALS_OK;
  }
  FILE* f = fopen(path, "rb");
  if (!f) return text_fail(g, MALS_IO_ERROR, std::string("cannot open ") + path);
  for (;;) {
    const size_t got = fread(buf, 1, buf_bytes, f);
    if (ferror(f)) {
      fclose(f);
      return text_fail(g, MALS_IO_ERROR, std::string("read error: ") + path);
    }
    const bool eof = got < buf_bytes;  // a short read without an error is the end of a regular file
    if (int rc = append_text_impl(g, buf, (int64_t)got, MALS_MEM_HOST, eof)) {
      fclose(f);
      return rc;
    }
    if (eof) break;
  }
  fclose(f);
  return MALS_OK;
}

}  // extern "C"

namespace {

struct InputFile {
  std::string path;
  int64_t mtime_ms, bytes;
};

// InputFilesReader.java:71-86: the input files of a directory in the order they are read; 1 when one is not a readable file
int list_input_files(mals_ingest g, const char* input_dir, std::vector<InputFile>* out) {
  DIR* d = opendir(input_dir);
  if (!d) return MALS_OK;  // listFiles() == null: "No input files", not an error (IFR:80-83)
  std::vector<InputFile> files;
  while (dirent* e = readdir(d)) {
    const std::string name(e->d_name);
    if (name == "." || name == ".." || !is_input_file_name(name)) continue;
    struct stat st;
    const std::string full = std::string(input_dir) + "/" + name;
    if (stat(full.c_str(), &st) != 0) continue;
    files.push_back({full, (int64_t)st.st_mtim.tv_sec * 1000 + st.st_mtim.tv_nsec / 1000000, (int64_t)st.st_size});  // File.lastModified(): ms
  }
  closedir(d);
  // ByLastModifiedComparator (ascending); Arrays.sort is stable over listFiles()'s unspecified order: by name here
  std::sort(files.begin(), files.end(), [](const InputFile& a, const InputFile& b) { return a.path < b.path; });
  std::stable_sort(files.begin(), files.end(), [](const InputFile& a, const InputFile& b) { return a.mtime_ms < b.mtime_ms; });
  for (const InputFile& f : files) {
    struct stat st;
    if (stat(f.path.c_str(), &st) != 0 || !S_ISREG(st.st_mode))
      return text_fail(g, MALS_IO_ERROR, f.path + " is not a readable file (FileInputStream would throw)");
  }
  *out = std::move(files);
  return MALS_OK;
}

bool splittable(const std::string& path) { return !ends_with(path, ".gz") && !ends_with(path, ".zip"); }

// the first line start at or after byte `at` of a plain file: byte 0, the byte after '\n', the byte after a '\r' that no
// '\n' follows (java.io.BufferedReader.readLine); `size` when no line starts there
int64_t next_line_start(const std::string& path, int64_t at, int64_t size) {
  if (at <= 0) return 0;
  if (at >= size) return size;
  FILE* f = fopen(path.c_str(), "rb");
  if (!f || fseeko(f, (off_t)(at - 1), SEEK_SET) != 0) {
    if (f) fclose(f);
    return size;   // the read of the piece reports the error
  }
  int prev = fgetc(f);
  int64_t p = at;
  for (; p < size; ++p) {
    const int c = fgetc(f);
    if (c == EOF) break;
    if (prev == '\n' || (prev == '\r' && c != '\n')) break;
    prev = c;
  }
  fclose(f);
  return std::min(p, size);
}

// bytes [b, e) of a plain file, the last block with end_of_file
int read_file_piece(mals_ingest g, const std::string& path, int64_t b, int64_t e) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return text_fail(g, MALS_IO_ERROR, std::string("cannot open ") + path);
  if (fseeko(f, (off_t)b, SEEK_SET) != 0) {
    fclose(f);
    return text_fail(g, MALS_IO_ERROR, std::string("read error: ") + path);
  }
  const size_t buf_bytes = std::min<size_t>(g->text_block_bytes, (size_t)64 << 20);
  if (buf_bytes > g->h_pinned.capacity()) ICHK(g, g->h_pinned.alloc(buf_bytes));
  uint8_t* buf = g->h_pinned.get();
  for (int64_t at = b;;) {
    const size_t want = (size_t)std::min<int64_t>((int64_t)buf_bytes, e - at);
    const size_t got = want ? fread(buf, 1, want, f) : 0;
    if (got != want) {
      fclose(f);
      return text_fail(g, MALS_IO_ERROR, std::string("read error: ") + path);
    }
    at += (int64_t)got;
    if (int rc = append_text_impl(g, buf, (int64_t)got, MALS_MEM_HOST, at == e)) {
      fclose(f);
      return rc;
    }
    if (at == e) break;
  }
  fclose(f);
  return MALS_OK;
}

}  // namespace

extern "C" {

int mals_ingest_read_dir(mals_ingest g, const char* input_dir, int32_t* n_files_read) {
  if (!g || !input_dir) return MALS_INVALID_ARG;
  if (n_files_read) *n_files_read = 0;
  if (g->spent) return fail(g, MALS_INVALID_ARG, "the ingest's records went into mals_group_ingest_finish: create a new ingest");
  if (g->text_failed) return fail(g, g->text_fail_code, g->text_fail_msg);
  std::vector<InputFile> files;
  if (int rc = list_input_files(g, input_dir, &files)) return rc;
  for (const InputFile& f : files) {
    if (int rc = mals_ingest_read_file(g, f.path.c_str())) return rc;
    if (n_files_read) ++*n_files_read;
  }
  return MALS_OK;
}

// The stream of mals_ingest_read_dir (files in its order, bytes in order) cut into n_shares pieces of about equal on-disk
// bytes.  A cut moves forward to the next line start of a plain file; a .gz / .zip file goes whole to the share in which its
// first byte falls.  Every share computes the same cuts from the same listing.
int mals_ingest_read_dir_share(mals_ingest g, const char* input_dir, int32_t share, int32_t n_shares, int32_t* n_files_read) {
  if (!g || !input_dir) return MALS_INVALID_ARG;
  if (n_files_read) *n_files_read = 0;
  if (n_shares < 1 || n_shares > MALS_SPLIT_MAX_SHARES || share < 0 || share >= n_shares) return fail(g, MALS_INVALID_ARG, "share: 0 <= share < n_shares <= 256");
  if (g->spent) return fail(g, MALS_INVALID_ARG, "the ingest's records went into mals_group_ingest_finish: create a new ingest");
  if (g->text_failed) return fail(g, g->text_fail_code, g->text_fail_msg);
  if (g->share != share) {
    if (int rc = mals_ingest_set_option(g, MALS_INGEST_OPT_SHARE, share)) return rc;
  }
  std::vector<InputFile> files;
  if (int rc = list_input_files(g, input_dir, &files)) return rc;
  std::vector<int64_t> start(files.size() + 1, 0);
  for (size_t i = 0; i < files.size(); ++i) start[i + 1] = start[i] + files[i].bytes;
  const int64_t total = start.back();
  // cut c (global byte offset) -> the line start at or after it
  auto adjust = [&](int64_t c) -> int64_t {
    if (c <= 0) return 0;
    if (c >= total) return total;
    const size_t i = (size_t)(std::upper_bound(start.begin(), start.end(), c) - start.begin()) - 1;   // start[i] <= c < start[i + 1]
    if (c == start[i]) return c;
    if (!splittable(files[i].path)) return start[i + 1];
    return start[i] + next_line_start(files[i].path, c - start[i], files[i].bytes);
  };
  const int64_t lo = adjust((int64_t)((__int128)total * share / n_shares));
  const int64_t hi = adjust((int64_t)((__int128)total * (share + 1) / n_shares));
  for (size_t i = 0; i < files.size(); ++i) {
    const int64_t fb = start[i], fe = start[i + 1];
    if (splittable(files[i].path)) {
      const int64_t b = std::max(lo, fb), e = std::min(hi, fe);
      if (e <= b) continue;
      ICHK(g, hipSetDevice(g->device));
      if (int rc = read_file_piece(g, files[i].path, b - fb, e - fb)) return rc;
    } else {
      // whole, in the share of its first byte (an empty file: the share whose range holds its offset)
      if (!(fb >= lo && (fb < hi || (fb == total && hi == total && share == n_shares - 1)))) continue;
      if (int rc = mals_ingest_read_file(g, files[i].path.c_str())) return rc;
    }
    if (n_files_read) ++*n_files_read;
  }
  return MALS_OK;
}

int mals_ingest_text_info(mals_ingest g, mals_ingest_text_info_t* out) {
  if (!g || !out || out->struct_size < (int32_t)sizeof(mals_ingest_text_info_t)) return MALS_INVALID_ARG;
  out->lines = g->lines;
  out->bad_lines = g->bad_lines;
  out->header_lines = g->header_lines;
  out->skipped_lines = g->skipped_lines;
  out->full_parser_lines = g->slow_lines;
  out->text_bytes = g->text_bytes;
  out->records = g->sharded ? g->shard_records : g->n;
  out->parse_ms = g->parse_ms;
  out->stage_ms = g->stage_ms;
  out->n_item_tag_ids = g->finished ? g->n_tag_ids[0] : -1;
  out->n_user_tag_ids = g->finished ? g->n_tag_ids[1] : -1;
  out->n_known_items = (g->finished && g->known_ptr.get()) ? g->n_known : -1;
  return MALS_OK;
}

int mals_ingest_get_tag_ids(mals_ingest g, int32_t which, int64_t* host_ids_out) {
  if (!g) return MALS_INVALID_ARG;
  if (which != MALS_ITEM_TAG_IDS && which != MALS_USER_TAG_IDS) return fail(g, MALS_INVALID_ARG, "which: MALS_ITEM_TAG_IDS or MALS_USER_TAG_IDS");
  if (!g->finished) return fail(g, MALS_INVALID_ARG, "mals_ingest_finish has not run");
  if (g->n_tag_ids[which] && !host_ids_out) return MALS_INVALID_ARG;
  ICHK(g, hipSetDevice(g->device));
  if (g->n_tag_ids[which])
    ICHK(g, hipMemcpy(host_ids_out, g->tag_ids[which].get(), sizeof(int64_t) * (size_t)g->n_tag_ids[which], hipMemcpyDeviceToHost));
  return MALS_OK;
}

int mals_ingest_get_known_items(mals_ingest g, int64_t* host_ptr, int32_t* host_item_idx) {
  if (!g) return MALS_INVALID_ARG;
  if (!g->finished || !g->known_ptr.get()) return fail(g, MALS_INVALID_ARG, "no known items: set MALS_INGEST_OPT_KNOWN_ITEMS before mals_ingest_finish");
  ICHK(g, hipSetDevice(g->device));
  const int64_t rows = g->sharded ? g->slice_rows[0] : g->n_users;
  if (host_ptr) ICHK(g, hipMemcpy(host_ptr, g->known_ptr.get(), sizeof(int64_t) * (size_t)(rows + 1), hipMemcpyDeviceToHost));
  if (host_item_idx && g->n_known)
    ICHK(g, hipMemcpy(host_item_idx, g->known_idx.get(), sizeof(int32_t) * (size_t)g->n_known, hipMemcpyDeviceToHost));
  return MALS_OK;
}

int mals_ingest_device_known_items(mals_ingest g, const int64_t** ptr, const int32_t** item_idx, int64_t* n_known) {
  if (!g) return MALS_INVALID_ARG;
  if (!g->finished || !g->known_ptr.get()) return fail(g, MALS_INVALID_ARG, "no known items: set MALS_INGEST_OPT_KNOWN_ITEMS before mals_ingest_finish");
  if (ptr) *ptr = g->known_ptr.get();
  if (item_idx) *item_idx = g->known_idx.get();
  if (n_known) *n_known = g->n_known;
  return MALS_OK;
}

}  // extern "C"
