// stream.cpp — the crate's streaming search (src/stream.rs) over the GPU search path.
//
// WindowReader (stream.rs:77-159): bytes are fed in the reader's read() pieces; once the buffer
// holds >= `window` bytes (or the input ended) a window is cut: its text is the buffer's valid
// UTF-8 prefix, and unless it is the last window it owns only the matches that start before the
// commit point — the byte start of the `overlap`-th grapheme from the end (overlap =
// max_match_graphemes + 1, stream.rs:256-258), found on the host from a short tail of the text;
// with too few graphemes the window grows and more input is awaited. The buffer then drops the
// committed prefix.
//
// Consecutive windows are collected into batches of about 32 MiB of text, and each batch is handed
// to one of `depth` (2) worker threads, batch k to worker k % depth. A worker owns a HIP stream and
// a device scratch set. An all-ASCII batch is staged once (H2D) and its windows searched in one
// launch, each as its own text (stream_windows_batch). A window's grapheme segmentation depends on
// where its text starts and ends, so the windows of other text cannot be grapheme ranges of one staged
// text; such a batch is uploaded once and searched as a fac::Batch whose document w is window w's text
// (stream_windows_docs). Windows overlap their neighbours and a batch's documents are disjoint, so a
// gather kernel copies every window's bytes, overlap included, into a second device buffer and
// writes the document offsets; the worker's Batch is restaged over it (UTF-8 check, is_ascii and UAX
// #29 from start-of-text per document, exactly a window's semantics; the windows are long documents,
// so they are segmented by 256-byte chunks, Batch::long_docs), the batch front runs the
// pre-filter where Prefiltered::search would, one search launch and the per-document rank and
// overlap walk, and the commit cut keeps each document's owned prefix, all on the device: only the
// owned records and their index come back. The same path takes an ASCII batch that
// stream_windows_batch declines (pre-filter tables that need the packed full scan). Only a batch of
// one window stages and searches it alone (H2D + device segmentation + folding). A pre-filtered
// stream (fac_stream_open_ex) searches every window's text as Prefiltered::search: the batched paths
// take the flag, a single window goes through prefiltered_view. Every window is ranked
// sorted().non_overlapping() and keeps the matches it owns (stream.rs:262-297). Batch k + 1's
// copies and kernels overlap batch k's (double buffering) while the host cuts the windows of batch
// k + 2. Finished batches are handed out strictly in window order.
//
// Whole-token matches (fac_stream_open_opts, StreamCore::boundaries): with a mask every
// window's raw records are filtered by the boundary rule before they are ranked, the start side
// looking to the left of the window into the stream's earlier text. The batched paths filter in HBM
// (boundary_kernels.hip stream_boundary_filter_kernel) over the task's text; a single window is
// filtered on the host (boundary_ok_after). The text before a task's first byte has left the
// buffer by then, so the reader keeps the stream's last kBoundaryCarry bytes as it drops the
// committed prefix (drop_prefix) and every task carries the kBoundaryCarry bytes before its base:
// the walk reads at most kBoundaryMaxSkip code points. With the mask 0 nothing of this runs.
//
// Replace mode (fac_replace_stream_*; stream.rs:465-517 + ReplaceCursor::emit_window, :645-705): a
// task's text stays on the device after the search, its owned records go back up, and the plan and
// copy kernels of replace_kernels.hip splice the task's output, which is copied to the host and
// handed out in stream order. A task's plan starts from its predecessor's cursor (`emitted`), so
// after its search a worker waits for task k - 1's plan; the searches still overlap.
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>
#include <new>
#include <stdexcept>
#include <thread>
#include <vector>

#include "fac_internal.h"

namespace fac {

// A batch of consecutive windows: text holds stream bytes [base, base + text.size()), window w is
// text[off, off + len) and owns the matches starting before off + commit.
struct StreamWin {
  uint64_t off, len, commit;
};
struct StreamTask {
  std::vector<uint8_t> text;
  uint64_t base = 0;
  // whole-token matches (StreamCore::boundaries): the stream's last bytes before `base`, at most
  // kBoundaryCarry of them, and whether the stream has text before those
  std::vector<uint8_t> before;
  bool more_before = false;
  std::vector<StreamWin> wins;
  std::vector<fac_match> res;  // owned matches of every window, in window order, absolute offsets
  std::vector<uint8_t> res_text;
  uint64_t seq = 0;          // dispatch order (replace mode: the cursor's order)
  std::vector<uint8_t> out;  // replace mode: the task's spliced output
  uint64_t applied = 0, skipped = 0;
  uint64_t searched = 0;  // start windows of the segments handed to the search launcher
  int rc = FAC_OK;
  std::string err;
  bool batched = false;  // searched in one pass (else window by window)
  bool done = false;
};

struct StreamWorker {
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  std::deque<StreamTask*> q;
  bool stop = false;
  hipStream_t stream = nullptr;
  ScratchSet scratch;
  // the window-documents batch, restaged in place from task to task and kept until stream_close: the
  // expanded text (~36 MiB for a 32 MiB task) and 12 bytes per grapheme of its non-ASCII windows
  WindowDocs docs;
};

namespace {

std::mutex g_done_mu;  // guards StreamTask::done across workers and the feeding thread
std::condition_variable g_done_cv;

// Search one window (text[off, off + len) of the task) and keep the matches it owns (stream.rs:262-297).
// shift: the stream offset the records are rebased to, less the window's offset in the task's text
int search_one_window(const StreamCore& s, StreamWorker& w, StreamTask& t, const StreamWin& win, uint64_t shift,
                      std::vector<fac_match>& owned, std::string& err) {
  Haystack h;
  int rc = stage_haystack(*s.e, t.text.data() + win.off, win.len, h, err, -1, w.stream);
  if (!rc) {
    SegDesc seg{};
    seg.text_base = 0;
    seg.n = h.n;
    seg.avail = h.n;
    seg.hay_len = h.len;
    seg.byte_base = 0;
    seg.w_begin = 0;
    seg.w_end = h.n;
    seg.ascii = h.ascii ? 1u : 0u;
    std::vector<fac_match> res;
    if (s.prefilter) {  // Prefiltered::search of the window's text (prefilter.rs:304-374)
      rc = prefiltered_view(*s.e, h, seg, s.threshold, w.stream, res, nullptr, err, &t.searched);
    } else {
      t.searched += seg.w_end - seg.w_begin;
      rc = launch_search(*s.e, h, {seg}, s.threshold, w.stream, res, nullptr, err);
    }
    if (!rc && s.boundaries && !res.empty()) {
      // whole-token matches: the host rule on the raw records, with the text to the window's left
      // (the task's text before it, then the task's carried context)
      std::vector<uint8_t> ctx;
      const uint8_t* before = nullptr;
      uint64_t bl = 0;
      if (win.off >= kBoundaryCarry) {
        before = t.text.data() + (win.off - kBoundaryCarry);
        bl = kBoundaryCarry;
      } else {
        const uint64_t take = std::min<uint64_t>(t.before.size(), kBoundaryCarry - win.off);
        ctx.assign(t.before.end() - (ptrdiff_t)take, t.before.end());
        ctx.insert(ctx.end(), t.text.begin(), t.text.begin() + (ptrdiff_t)win.off);
        before = ctx.data();
        bl = ctx.size();
      }
      const bool more = t.base + win.off > bl;  // else the context's front is byte 0 of the stream
      size_t kept = 0;
      for (const fac_match& m : res) {
        const int ok = boundary_ok_after(before, bl, more, t.text.data() + win.off, win.len, m.start, m.end, s.boundaries);
        if (ok < 0) {
          err = "a stream window's boundary context is too short";
          rc = FAC_E_INTERNAL;
          break;
        }
        if (ok) res[kept++] = m;
      }
      res.resize(kept);
    }
    if (!rc) rc = apply_matches(*s.e, res, /*Default*/ 1, /*NonOverlapping*/ 1, nullptr, err);
    if (!rc)
      for (const fac_match& m : res) {
        if (m.start >= win.commit) continue;
        fac_match a = m;
        a.start += shift + win.off;
        a.end += shift + win.off;
        owned.push_back(a);
      }
  }
  free_haystack(h);
  return rc;
}

// Replace mode: the splice of a task. d_text: the task's text if the search left it on the device,
// else it is uploaded here. owned / win_off: the task's owned records at offsets of its text, in
// window order, and their CSR index. Waits for the predecessor's cursor, plans from it, copies the
// output back and passes the cursor on -- also when the task failed, so no successor waits forever.
void splice_task(StreamCore& s, StreamWorker& w, StreamTask& t, const uint8_t* d_text, std::vector<fac_match>& owned,
                 const std::vector<uint64_t>& win_off) {
  void* up = nullptr;
  if (!t.rc && !d_text && !t.text.empty()) {
    hipError_t he = hipSuccess;
    up = call_scratch_take(t.text.size(), w.stream, &he);
    if (he != hipSuccess || !up) {
      up = nullptr;
      t.rc = FAC_E_OOM;
      t.err = std::string("hipMalloc: ") + hipGetErrorString(he);
    } else if (hipMemcpyAsync(up, t.text.data(), t.text.size(), hipMemcpyHostToDevice, w.stream) != hipSuccess) {
      t.rc = FAC_E_HIP;
      t.err = "upload of a stream task's text failed";
    }
    d_text = static_cast<const uint8_t*>(up);
  }
  uint64_t emitted = 0;
  {
    std::unique_lock<std::mutex> lk(s.cur_mu);
    s.cur_cv.wait(lk, [&] { return s.cur_seq == t.seq; });
    emitted = s.cur_emitted;
    if (s.cur_failed && !t.rc) {
      t.rc = FAC_E_INTERNAL;
      t.err = "an earlier task of the stream failed";
    }
  }
  if (!t.rc) {
    std::vector<uint64_t> commit(t.wins.size());
    for (size_t i = 0; i < t.wins.size(); ++i) commit[i] = t.wins[i].off + t.wins[i].commit;
    StreamReplacePlan plan;
    t.rc = replace_stream_plan_device(*s.table, owned, win_off, commit, emitted - t.base, w.stream, plan, t.err);
    if (!t.rc && plan.total >= (1ull << kDocTagShift)) {
      t.rc = FAC_E_UNSUPPORTED;
      t.err = "a stream task's output would hold 2^40 bytes or more";
    }
    if (!t.rc && plan.total) {
      hipError_t he = hipSuccess;
      void* d_out = call_scratch_take(plan.total, w.stream, &he);
      if (he != hipSuccess || !d_out) {
        t.rc = FAC_E_OOM;
        t.err = std::string("hipMalloc: ") + hipGetErrorString(he);
      } else {
        t.out.resize(plan.total);
        t.rc = replace_stream_copy_device(d_text, *s.table, plan, static_cast<uint8_t*>(d_out), t.err);
        if (!t.rc && (hipMemcpyAsync(t.out.data(), d_out, plan.total, hipMemcpyDeviceToHost, w.stream) != hipSuccess ||
                      hipStreamSynchronize(w.stream) != hipSuccess)) {
          t.rc = FAC_E_HIP;
          t.err = "copy of a stream task's output failed";
        }
        call_scratch_give(d_out, w.stream);
      }
    }
    if (!t.rc) {
      emitted = t.base + plan.e_out;
      t.applied = plan.n_replaced;
      t.skipped = plan.n_skipped;
    }
  }
  if (up) {
    (void)hipStreamSynchronize(w.stream);  // (an error path may leave the upload in flight)
    call_scratch_give(up, w.stream);
  }
  {
    std::lock_guard<std::mutex> lk(s.cur_mu);
    s.cur_emitted = emitted;
    s.cur_failed = s.cur_failed || t.rc != FAC_OK;
    s.cur_seq = t.seq + 1;
  }
  s.cur_cv.notify_all();
}

// Search a task of windows. A task of one window stages and searches it alone. Any other task is
// searched in one pass: all-ASCII text is staged once and its windows searched as one launch over
// their union (stream_windows_batch: each window its own text, ranked and cut per window); text with
// anything else, or a task that path declines, is uploaded once and searched as a batch whose
// documents are the windows' texts (stream_windows_docs: a window's grapheme segmentation depends on
// where its text starts and ends, so every window is staged as a document of its own).
void run_window_task(StreamCore& s, StreamWorker& w, StreamTask& t) {
  const bool replace = s.table != nullptr;
  // replace mode keeps the records at offsets of the task's text, which the splice reads
  const uint64_t shift = replace ? 0 : t.base;
  std::vector<fac_match> owned;
  std::vector<uint64_t> win_off(t.wins.size() + 1, 0);
  bool batched = false, staged = false;
  Haystack h;  // the whole task's text (the ASCII path); resident until the splice is done
  void* up = nullptr;  // the same for the window-documents path
  const bool multi = t.wins.size() > 1;
  StreamBoundary sb;
  sb.sides = s.boundaries;
  sb.before = t.before.data();
  sb.before_len = (uint32_t)t.before.size();
  sb.more_before = t.more_before;
  std::vector<uint64_t> wins(multi ? 4 * t.wins.size() : 0);
  for (size_t i = 0; multi && i < t.wins.size(); ++i) {
    wins[4 * i] = t.wins[i].off;
    wins[4 * i + 1] = t.wins[i].off + t.wins[i].len;
    wins[4 * i + 2] = t.wins[i].commit;
    wins[4 * i + 3] = shift + t.wins[i].off;
  }
  if (multi && ascii_only(t.text.data(), t.text.size())) {
    t.rc = stage_haystack(*s.e, t.text.data(), t.text.size(), h, t.err, 1, w.stream);
    staged = true;
    if (!t.rc) {
      uint64_t searched = 0;
      const int rc = stream_windows_batch(*s.e, h, wins.data(), t.wins.size(), s.threshold, s.prefilter, w.stream, owned,
                                          nullptr, t.err, &win_off, &searched, &sb);
      if (rc != FAC_E_UNSUPPORTED) {  // (unsupported: pre-filter tables that need the packed full scan)
        t.rc = rc;
        t.searched += searched;
        batched = true;
      }
    }
    if (t.rc) batched = true;  // a staging failure is the task's error
  }
  if (multi && !batched && s.window_docs) {
    const uint8_t* d_text = staged ? h.d_utf8 : nullptr;
    if (!d_text) {
      hipError_t he = hipSuccess;
      up = call_scratch_take(t.text.size(), w.stream, &he);
      if (he != hipSuccess || !up) {
        up = nullptr;
        t.rc = FAC_E_OOM;
        t.err = std::string("hipMalloc: ") + hipGetErrorString(he);
      } else if (hipMemcpyAsync(up, t.text.data(), t.text.size(), hipMemcpyHostToDevice, w.stream) != hipSuccess) {
        t.rc = FAC_E_HIP;
        t.err = "upload of a stream task's text failed";
      }
      d_text = static_cast<const uint8_t*>(up);
    }
    if (!t.rc) {
      uint64_t searched = 0;
      const int rc = stream_windows_docs(*s.e, w.docs, d_text, t.text.size(), wins.data(), t.wins.size(), s.threshold,
                                         s.prefilter, w.stream, owned, t.err, win_off, &searched, &sb);
      if (rc != FAC_E_UNSUPPORTED) {  // (unsupported: more windows or bytes than a batch holds)
        t.rc = rc;
        t.searched += searched;
        batched = true;
      }
    }
    if (t.rc) batched = true;
  }
  if (!batched) {
    owned.clear();
    for (size_t i = 0; i < t.wins.size(); ++i) {
      win_off[i] = owned.size();
      if ((t.rc = search_one_window(s, w, t, t.wins[i], shift, owned, t.err))) break;
    }
    win_off[t.wins.size()] = owned.size();
  }
  t.batched = batched;
  if (replace) {
    const uint8_t* resident = t.rc ? nullptr : staged ? h.d_utf8 : static_cast<const uint8_t*>(up);
    splice_task(s, w, t, resident, owned, win_off);
  } else if (!t.rc) {
    for (const fac_match& m : owned) {
      t.res.push_back(m);
      t.res_text.insert(t.res_text.end(), t.text.begin() + (ptrdiff_t)(m.start - t.base),
                        t.text.begin() + (ptrdiff_t)(m.end - t.base));
    }
  }
  if (staged) free_haystack(h);
  if (up) {
    (void)hipStreamSynchronize(w.stream);  // (an error path may leave the upload in flight)
    call_scratch_give(up, w.stream);
  }
  std::vector<uint8_t>().swap(t.text);
}

// Replace mode, after a task threw: if its splice did not pass the cursor on, step over the task once
// its predecessor has finished (it will: it was dispatched earlier, to the other worker), so that the
// successor does not wait forever.
void pass_cursor(StreamCore& s, const StreamTask& t) {
  if (!s.table) return;
  {
    std::unique_lock<std::mutex> lk(s.cur_mu);
    s.cur_cv.wait(lk, [&] { return s.cur_seq >= t.seq; });
    if (s.cur_seq > t.seq) return;
    s.cur_failed = true;
    s.cur_seq = t.seq + 1;
  }
  s.cur_cv.notify_all();
}

void worker_loop(StreamCore* s, StreamWorker* w) {
  (void)hipSetDevice(s->e->device);
  scratch_bind(&w->scratch);
  for (;;) {
    StreamTask* t = nullptr;
    {
      std::unique_lock<std::mutex> lk(w->mu);
      w->cv.wait(lk, [&] { return w->stop || !w->q.empty(); });
      if (w->q.empty()) break;  // stop requested and nothing queued
      t = w->q.front();
      w->q.pop_front();
    }
    try {  // an allocation failure becomes the window's error code, not std::terminate
      run_window_task(*s, *w, *t);
    } catch (const std::bad_alloc&) {
      t->rc = FAC_E_OOM;
      t->err = "out of host memory while searching a stream window";
      pass_cursor(*s, *t);
    } catch (const std::exception& ex) {
      t->rc = FAC_E_INTERNAL;
      t->err = std::string("stream window: ") + ex.what();
      pass_cursor(*s, *t);
    }
    {
      std::lock_guard<std::mutex> lk(g_done_mu);
      t->done = true;
    }
    g_done_cv.notify_all();
  }
  scratch_bind(nullptr);
}

// Hand out finished windows in order; `all`: wait for every window in flight.
int collect(StreamCore& s, bool all, std::string& err) {
  while (!s.inflight.empty()) {
    StreamTask* t = s.inflight.front();
    {
      std::unique_lock<std::mutex> lk(g_done_mu);
      if (!t->done && !all) return FAC_OK;
      g_done_cv.wait(lk, [&] { return t->done; });
    }
    s.inflight.erase(s.inflight.begin());
    if (!t->wins.empty()) s.handed = t->base + t->wins.back().off + t->wins.back().commit;
    if (t->rc && !s.failed) {
      s.failed = t->rc;
      s.fail_msg = t->err;
    }
    s.ready.insert(s.ready.end(), t->res.begin(), t->res.end());
    s.ready_text.insert(s.ready_text.end(), t->res_text.begin(), t->res_text.end());
    if (!s.failed) {
      s.ready_out.insert(s.ready_out.end(), t->out.begin(), t->out.end());
      s.written += t->out.size();
      s.applied += t->applied;
      s.skipped += t->skipped;
    }
    s.windows_searched += t->searched;
    ++(t->batched ? s.tasks_batched : s.tasks_single);
    delete t;
  }
  if (s.failed) {
    err = s.fail_msg;
    return s.failed;
  }
  return FAC_OK;
}

int dispatch(StreamCore& s, StreamTask* t, std::string& err) {
  // the worker of this window finished its previous window (at most `depth` in flight)
  while (s.inflight.size() >= StreamCore::depth) {
    StreamTask* f = s.inflight.front();
    {
      std::unique_lock<std::mutex> lk(g_done_mu);
      g_done_cv.wait(lk, [&] { return f->done; });
    }
    if (int rc = collect(s, false, err)) {
      delete t;
      return rc;
    }
  }
  t->seq = s.seq;
  StreamWorker* w = s.workers[s.seq++ % StreamCore::depth];
  s.inflight.push_back(t);
  {
    std::lock_guard<std::mutex> lk(w->mu);
    w->q.push_back(t);
  }
  w->cv.notify_one();
  return FAC_OK;
}

// Cut windows while the buffer allows (next_window, stream.rs:102-158). The crate's reader reads
// 64 KiB pieces until it holds >= window bytes, so a window's text is the carry left by the previous
// window plus whole 64 KiB reads (the last one partial at the end of the input); fed in larger pieces,
// the buffer is cut the same way. Consecutive windows join the pending batch, dispatched once it holds
// kBatchBytes of text or the input ends. (StreamCore::read: the read size, 64 KiB.)

int flush_batch(StreamCore& s, std::string& err) {
  if (!s.pending) return FAC_OK;
  StreamTask* t = s.pending;
  s.pending = nullptr;
  return dispatch(s, t, err);
}

// Whole-token matches: s.tail keeps the stream's last kBoundaryCarry bytes before buf[0] as the
// committed prefix buf[0, at) is dropped, so a task that begins later still has its left context.
void drop_prefix(StreamCore& s, uint64_t at) {
  if (s.boundaries && at) {
    if (at >= kBoundaryCarry) {
      s.tail.assign(s.buf.begin() + (ptrdiff_t)(at - kBoundaryCarry), s.buf.begin() + (ptrdiff_t)at);
    } else {
      s.tail.insert(s.tail.end(), s.buf.begin(), s.buf.begin() + (ptrdiff_t)at);
      if (s.tail.size() > kBoundaryCarry) s.tail.erase(s.tail.begin(), s.tail.end() - (ptrdiff_t)kBoundaryCarry);
    }
  }
  s.buf.erase(s.buf.begin(), s.buf.begin() + (ptrdiff_t)at);
}

int pump(StreamCore& s, bool eof, std::string& err) {
  // the buffer's unconsumed bytes start at `at` (the committed prefix is dropped once per call: an
  // erase per window moved the rest of a large feed again for every window)
  uint64_t at = 0;
  while (!s.done) {
    const uint8_t* b = s.buf.data() + at;
    const uint64_t avail = s.buf.size() - at;
    const uint64_t want = s.carry >= s.window ? s.carry : s.carry + (s.window - s.carry + s.read - 1) / s.read * s.read;
    if (!eof && avail < want) break;  // the reader would block for more input
    const uint64_t len = std::min(avail, want);
    // the valid UTF-8 prefix of the window's bytes; bytes a previous window already validated (up to
    // valid_end, a character boundary) are not scanned again
    const uint64_t vfrom = std::min<uint64_t>(len, s.valid_end > s.base ? s.valid_end - s.base : 0);
    const uint64_t valid = vfrom + utf8_valid_prefix(b + vfrom, len - vfrom);
    s.valid_end = s.base + valid;
    const bool last = len < s.window;  // reached only at end of input
    uint64_t commit = valid;
    if (!last) {
      // byte start of the overlap-th grapheme from the end; none or 0: grow and read more
      uint64_t off = 0;
      if (!nth_grapheme_from_end(b, valid, s.overlap, off) || off == 0) {
        s.window += std::max<uint64_t>(s.window, 64 * 1024);
        continue;  // (at end of input the next round is the last window)
      }
      commit = off;
    }
    if (!s.pending) {
      s.pending = new StreamTask();
      s.pending->base = s.base;
      if (s.boundaries) {  // the last bytes before the task: of buf[0, at), then of the saved tail
        std::vector<uint8_t>& c = s.pending->before;
        const uint64_t from_buf = std::min<uint64_t>(at, kBoundaryCarry);
        const uint64_t from_tail = std::min<uint64_t>(s.tail.size(), kBoundaryCarry - from_buf);
        c.assign(s.tail.end() - (ptrdiff_t)from_tail, s.tail.end());
        c.insert(c.end(), s.buf.begin() + (ptrdiff_t)(at - from_buf), s.buf.begin() + (ptrdiff_t)at);
        s.pending->more_before = s.base > c.size();
      }
    }
    StreamTask* t = s.pending;
    const uint64_t off = s.base - t->base;  // the window's first byte in the batch text
    if (off + valid > t->text.size()) t->text.insert(t->text.end(), b + (t->text.size() - off), b + valid);
    t->wins.push_back(StreamWin{off, valid, commit});
    if (last) {
      s.done = true;
      break;
    }
    at += commit;
    s.base += commit;
    s.carry = len - commit;
    if (t->text.size() >= s.batch_bytes)
      if (int rc = flush_batch(s, err)) {
        drop_prefix(s, at);
        return rc;
      }
  }
  drop_prefix(s, at);
  if (eof || s.done)
    if (int rc = flush_batch(s, err)) return rc;
  return collect(s, eof, err);
}

}  // namespace

int stream_feed(StreamCore& s, const uint8_t* data, uint64_t len, bool eof, std::string& err) {
  if (s.done) return collect(s, true, err);
  if (len) {
    s.buf.insert(s.buf.end(), data, data + len);
    s.total += len;
  }
  return pump(s, eof, err);
}

StreamCore* stream_open(const Engine& e, float threshold, uint64_t window, const ReplaceTable* table, bool prefilter,
                        int boundaries) {
  StreamCore* s = new StreamCore();
  s->e = &e;
  s->boundaries = boundaries;
  s->threshold = threshold;
  s->table = table;
  s->prefilter = prefilter;
  if (const char* v = diag_env("FAC_STREAM_BATCH_BYTES"))  // diagnostics: task boundaries at small sizes
    s->batch_bytes = std::max<uint64_t>(1, std::strtoull(v, nullptr, 10));
  if (const char* v = diag_env("FAC_STREAM_READ_BYTES"))  // diagnostics: the reader's read size, many windows of a small input
    s->read = std::max<uint64_t>(1, std::strtoull(v, nullptr, 10));
  if (const char* v = diag_env("FAC_STREAM_WINDOW_DOCS"))  // diagnostics: 0 = non-ASCII tasks window by window
    s->window_docs = std::strtoull(v, nullptr, 10) != 0;
  if (window) s->window = window;
  s->overlap = e.max_match_graphemes + 1;  // stream_overlap (stream.rs:256-258)
  (void)hipSetDevice(e.device);
  for (uint32_t i = 0; i < StreamCore::depth; ++i) {
    StreamWorker* w = new StreamWorker();
    (void)hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking);
    w->th = std::thread(worker_loop, s, w);
    s->workers[i] = w;
  }
  return s;
}

void stream_close(StreamCore* s) {
  std::string err;
  delete s->pending;  // windows cut but never dispatched (an abandoned stream)
  s->pending = nullptr;
  (void)collect(*s, true, err);  // windows still in flight
  for (StreamWorker* w : s->workers) {
    if (!w) continue;
    {
      std::lock_guard<std::mutex> lk(w->mu);
      w->stop = true;
    }
    w->cv.notify_one();
    w->th.join();
    (void)hipSetDevice(s->e->device);
    scratch_free(w->scratch);
    free_batch(w->docs.b);
    if (w->stream) {
      call_scratch_release_stream(w->stream);
      (void)hipStreamDestroy(w->stream);
    }
    delete w;
  }
  delete s;
}

uint64_t stream_committed(const StreamCore& s) { return s.handed; }

}  // namespace fac
