// lda_api.cpp -- C ABI of include/kaldi_lda.h: the handle (host statistics
// plus the device accumulators of lda_stats.hip), LdaEstimate's accumulator
// files, acc-lda over an egs archive and the estimator's entry points.
#include "kaldi_lda.h"

#include <algorithm>
#include <cctype>
#include <fstream>
#include <iomanip>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "common.h"
#include "egs.h"
#include "elementwise.h"
#include "kaldi_io.h"
#include "lda.h"
#include "nnet_handle.h"
#include "test_hooks.h"

namespace kio = kctc::kio;

namespace {

// grow-only device buffer of the archive driver
struct Buf {
  void *p = nullptr;
  size_t bytes = 0;
  ~Buf() {
    if (p) (void)hipFree(p);
  }
  void ensure(size_t b, hipStream_t s) {
    if (b <= bytes) return;
    if (p) {
      KCTC_HIP_CHECK(hipStreamSynchronize(s));
      KCTC_HIP_CHECK(hipFree(p));
      p = nullptr;
      bytes = 0;
    }
    KCTC_HIP_CHECK(hipMalloc(&p, b));
    bytes = b;
  }
  float *f() const { return static_cast<float *>(p); }
};

}  // namespace

// The statistics of a handle are host sums (set_stats / read) plus what the
// device has accumulated; only accumulate and acc_egs touch the device.
struct kctcLda_ {
  int D, C;
  std::vector<double> zero, first, second;  // second: full D x D, symmetric
  kctc::lda::DeviceStats dev;
  hipStream_t stream = nullptr;  // acc_egs
  Buf raw, padded, spliced, ids;
  kctcLda_(int dim, int classes, int device)
      : D(dim), C(classes), zero(classes, 0.0), first((size_t)classes * dim, 0.0), second((size_t)dim * dim, 0.0),
        dev(dim, classes, device) {}
  ~kctcLda_() {
    if (stream) {
      (void)hipStreamSynchronize(stream);
      (void)hipStreamDestroy(stream);
    }
  }
  void Get(std::vector<double> *z, std::vector<double> *f, std::vector<double> *s) {
    *z = zero;
    *f = first;
    *s = second;
    dev.AddTo(z->data(), f->data(), s->data());
    for (int i = 0; i < D; i++)
      for (int j = 0; j < i; j++) (*s)[(size_t)j * D + i] = (*s)[(size_t)i * D + j];
  }
  void Set(const double *z, const double *f, const double *s, bool add) {
    if (!add) {
      dev.Zero();
      std::fill(zero.begin(), zero.end(), 0.0);
      std::fill(first.begin(), first.end(), 0.0);
      std::fill(second.begin(), second.end(), 0.0);
    }
    for (int c = 0; c < C; c++) zero[c] += z[c];
    for (size_t i = 0; i < first.size(); i++) first[i] += f[i];
    for (int i = 0; i < D; i++)
      for (int j = 0; j <= i; j++) {
        second[(size_t)i * D + j] += s[(size_t)i * D + j];
        second[(size_t)j * D + i] = second[(size_t)i * D + j];
      }
  }
};

// PackedMatrix<float>::Write / Read (src/matrix/packed-matrix.cc): "FP" n raw |
// "[\n a \n b c ]\n", the lower triangle row by row
static void write_packed(std::ostream &os, bool binary, const std::vector<float> &p, int n) {
  if (binary) {
    kio::WriteToken(os, binary, "FP");
    kio::WriteInt(os, binary, n);
    os.write(reinterpret_cast<const char *>(p.data()), 4 * p.size());
    return;
  }
  os << "[\n";
  size_t i = 0;
  for (int r = 0; r < n; r++) {
    for (int c = 0; c <= r; c++) os << std::setprecision(9) << p[i++] << ' ';
    os << (r == n - 1 ? "]\n" : "\n");
  }
}
static std::vector<double> read_packed(std::istream &is, bool binary, int n) {
  const size_t num = (size_t)n * (n + 1) / 2;
  std::vector<double> p;
  if (binary) {
    const std::string t = kio::ReadToken(is, binary);
    if (kio::ReadInt(is, binary) != n) kio::Fail("PackedMatrix::Read: size mismatch");
    p.resize(num);
    if (t == "FP") {
      std::vector<float> f(num);
      is.read(reinterpret_cast<char *>(f.data()), 4 * num);
      std::copy(f.begin(), f.end(), p.begin());
    } else if (t == "DP") {
      is.read(reinterpret_cast<char *>(p.data()), 8 * num);
    } else {
      kio::Fail("PackedMatrix::Read: expected FP or DP, got " + t);
    }
    if (!is) kio::Fail("PackedMatrix::Read: truncated");
    return p;
  }
  std::string s;
  is >> s;
  if (s != "[") kio::Fail("PackedMatrix::Read: expected [, got " + s);
  while (is >> s && s != "]") p.push_back((double)std::stof(s));  // an SpMatrix<float>
  if (s != "]" || p.size() != num) kio::Fail("PackedMatrix::Read: size mismatch");
  return p;
}

static void write_accs(kctcLda_t h, const char *path, bool binary) {
  std::vector<double> z, f, s;
  h->Get(&z, &f, &s);
  const int D = h->D, C = h->C;
  // the variances are stored relative to the class means (LdaEstimate::Write)
  for (int c = 0; c < C; c++) {
    if (z[c] == 0.0) continue;
    const double *fc = &f[(size_t)c * D];
    const double inv = -1.0 / z[c];
    for (int i = 0; i < D; i++)
      for (int j = 0; j <= i; j++) s[(size_t)i * D + j] += inv * fc[i] * fc[j];
  }
  std::vector<float> zf(z.begin(), z.end()), ff(f.begin(), f.end()), pf;
  pf.reserve((size_t)D * (D + 1) / 2);
  for (int i = 0; i < D; i++)
    for (int j = 0; j <= i; j++) pf.push_back((float)s[(size_t)i * D + j]);
  kio::WriteFile(path, binary, [&](std::ostream &os) {
    kio::WriteToken(os, binary, "<LDAACCS>");
    kio::WriteToken(os, binary, "<VECSIZE>");
    kio::WriteInt(os, binary, D);
    kio::WriteToken(os, binary, "<NUMCLASSES>");
    kio::WriteInt(os, binary, C);
    kio::WriteToken(os, binary, "<ZERO_ACCS>");
    kio::WriteFloatVector(os, binary, zf.data(), C, 9);
    kio::WriteToken(os, binary, "<FIRST_ACCS>");
    kio::WriteFloatMatrix(os, binary, ff.data(), C, D, 9);
    kio::WriteToken(os, binary, "<SECOND_ACCS>");
    write_packed(os, binary, pf, D);
    kio::WriteToken(os, binary, "</LDAACCS>");
  });
}

static void read_accs(kctcLda_t h, const char *path, bool add) {
  std::istringstream is(kio::ReadFile(path));
  const bool binary = kio::InitInput(is);
  kio::ExpectToken(is, binary, "<LDAACCS>");
  kio::ExpectToken(is, binary, "<VECSIZE>");
  const int D = kio::ReadInt(is, binary);
  kio::ExpectToken(is, binary, "<NUMCLASSES>");
  const int C = kio::ReadInt(is, binary);
  if (D != h->D || C != h->C)
    throw std::invalid_argument("LdaEstimate::Read: the file holds " + std::to_string(C) + " classes of dimension " +
                                std::to_string(D) + ", the handle " + std::to_string(h->C) + " of " +
                                std::to_string(h->D));
  std::vector<double> z(C, 0.0), f((size_t)C * D, 0.0), s((size_t)D * D, 0.0);
  for (std::string tok = kio::ReadToken(is, binary); tok != "</LDAACCS>"; tok = kio::ReadToken(is, binary)) {
    if (tok == "<ZERO_ACCS>") {
      const std::vector<float> v = kio::ReadFloatVector(is, binary);
      if ((int)v.size() != C) kio::Fail("<ZERO_ACCS>: wrong size");
      std::copy(v.begin(), v.end(), z.begin());
    } else if (tok == "<FIRST_ACCS>") {
      int r = 0, c = 0;
      const std::vector<float> m = kio::ReadFloatMatrix(is, binary, &r, &c);
      if (r != C || c != D) kio::Fail("<FIRST_ACCS>: wrong size");
      std::copy(m.begin(), m.end(), f.begin());
    } else if (tok == "<SECOND_ACCS>") {
      const std::vector<double> p = read_packed(is, binary, D);
      size_t k = 0;
      for (int i = 0; i < D; i++)
        for (int j = 0; j <= i; j++) s[(size_t)i * D + j] = p[k++];
      // back to plain second moments, with the counts and sums read before it
      for (int c = 0; c < C; c++) {
        if (z[c] == 0.0) continue;
        const double *fc = &f[(size_t)c * D];
        const double inv = 1.0 / z[c];
        for (int i = 0; i < D; i++)
          for (int j = 0; j <= i; j++) s[(size_t)i * D + j] += inv * fc[i] * fc[j];
      }
    } else {
      kio::Fail("LdaEstimate::Read: unexpected token " + tok);
    }
  }
  h->Set(z.data(), f.data(), s.data(), add);
}

// binary "ark:" table of Int32Vector, whole, by key
static std::map<std::string, std::vector<int32_t>> read_ali_table(const char *rspecifier) {
  std::string path = rspecifier;
  const auto colon = path.find(':');
  if (colon != std::string::npos) {
    KCTC_REQUIRE(path.compare(0, 3, "ark") == 0, "only ark: specifiers are supported");
    path = path.substr(colon + 1);
  }
  std::ifstream is(path, std::ios::binary);
  if (!is) throw std::runtime_error("cannot open alignment archive " + path);
  std::map<std::string, std::vector<int32_t>> table;
  for (;;) {
    int c;
    while ((c = is.get()) != EOF && isspace(c)) {
    }
    if (c == EOF) break;
    std::string key(1, (char)c);
    while ((c = is.get()) != EOF && c != ' ') key.push_back((char)c);
    if (c == EOF || is.get() != '\0' || is.get() != 'B')
      throw std::runtime_error(path + ": entry " + key + " is not a binary Int32Vector");
    table[key] = kio::ReadIntVector(is, true);
  }
  return table;
}

// the class of every frame of one alignment under blank_policy; -1: not counted
static std::vector<int32_t> frame_classes(const std::vector<int32_t> &ali, int policy, int C) {
  std::vector<int32_t> ids(ali);
  for (int32_t v : ali)
    if (v < -1 || v >= C) throw std::invalid_argument("an alignment entry is outside [-1, num_classes)");
  if (policy == KCTC_LDA_BLANK_SKIP) {
    for (auto &v : ids)
      if (v == 0) v = -1;
  } else if (policy == KCTC_LDA_BLANK_FILL) {
    int32_t next = -1;  // the next non-blank label; for the trailing blanks, the last one
    for (size_t t = ali.size(); t-- > 0;)
      if (ali[t] > 0) {
        next = ali[t];
        break;
      }
    for (size_t t = ali.size(); t-- > 0;) {
      if (ali[t] > 0) next = ali[t];
      else if (ali[t] == 0) ids[t] = next;
    }
  }
  return ids;
}

static long g_batch_rows = 8192;  // kctc_lda_test_batch_rows

static void acc_egs(kctcLda_t h, const char *egs_rspecifier, const char *ali_rspecifier, const int *context,
                    int n_context, int policy, long *num_used, long *num_no_ali, long *num_mismatch,
                    long *num_frames) {
  KCTC_REQUIRE(n_context >= 1 && n_context <= kctc::kMaxSplice, "kctc_lda_acc_egs: 1..32 context offsets");
  KCTC_REQUIRE(policy >= KCTC_LDA_BLANK_SKIP && policy <= KCTC_LDA_BLANK_FILL, "kctc_lda_acc_egs: bad blank_policy");
  for (int k = 1; k < n_context; k++)
    KCTC_REQUIRE(context[k] > context[k - 1], "kctc_lda_acc_egs: the context offsets must increase");
  KCTC_REQUIRE(h->D % n_context == 0, "kctc_lda_acc_egs: dim is not a multiple of the number of context offsets");
  const int fdim = h->D / n_context;
  const int left = std::max(0, -context[0]), right = std::max(0, context[n_context - 1]);
  const int ns = 1 + left + right;
  const auto table = read_ali_table(ali_rspecifier);
  KCTC_HIP_CHECK(hipSetDevice(h->dev.device()));
  if (!h->stream) KCTC_HIP_CHECK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  hipStream_t st = h->stream;

  const long kBatchRows = g_batch_rows;  // spliced rows per accumulate call (plus the last example's)
  struct Utt {
    long raw_off;  // first row in the batch's raw rows
    int rows, first, frames;
  };
  std::vector<Utt> utts;
  std::vector<float> raw;
  std::vector<int32_t> ids;
  long used = 0, no_ali = 0, mismatch = 0, frames = 0;
  auto flush = [&]() {
    if (utts.empty()) return;
    const long R = (long)ids.size();
    int max_rows = 0;
    for (const Utt &u : utts) max_rows = std::max(max_rows, u.rows);
    h->raw.ensure(sizeof(float) * raw.size(), st);
    h->padded.ensure(sizeof(float) * (size_t)max_rows * ns * fdim, st);
    h->spliced.ensure(sizeof(float) * (size_t)R * h->D, st);
    h->ids.ensure(sizeof(int32_t) * (size_t)R, st);
    KCTC_HIP_CHECK(hipMemcpyAsync(h->raw.p, raw.data(), sizeof(float) * raw.size(), hipMemcpyHostToDevice, st));
    KCTC_HIP_CHECK(hipMemcpyAsync(h->ids.p, ids.data(), sizeof(int32_t) * (size_t)R, hipMemcpyHostToDevice, st));
    long out_row = 0;
    for (const Utt &u : utts) {
      // every example padded at its own ends, then its output frames spliced into the batch
      kctc::pad_splice_input(st, h->raw.f() + (size_t)u.raw_off * fdim, u.rows, fdim, left, ns, h->padded.f());
      kctc::splice_rows(st, h->padded.f() + (size_t)u.first * ns * fdim, fdim, ns, u.frames, context, n_context, left,
                        0, h->spliced.f() + (size_t)out_row * h->D);
      out_row += u.frames;
    }
    KCTC_HIP_CHECK(hipGetLastError());
    h->dev.Accumulate(st, h->spliced.f(), static_cast<const int *>(h->ids.p), nullptr, R);
    KCTC_HIP_CHECK(hipStreamSynchronize(st));  // the host vectors are reused
    utts.clear();
    raw.clear();
    ids.clear();
  };

  kctc::egs::ArchiveReader reader(egs_rspecifier);
  for (;;) {
    kctc::egs::Example eg;
    if (!reader.Next(&eg)) break;
    const auto it = table.find(eg.key);
    if (it == table.end()) {
      no_ali++;
      continue;
    }
    const int rows = eg.NumFrames(), L = (int)it->second.size();
    KCTC_REQUIRE(eg.NumCols() == fdim, "kctc_lda_acc_egs: feature dimension * context offsets != dim");
    if (L == 0 || eg.left_context < 0 || (long)eg.left_context + L > rows) {
      mismatch++;
      continue;
    }
    const std::vector<int32_t> cls = frame_classes(it->second, policy, h->C);
    utts.push_back(Utt{(long)(raw.size() / fdim), rows, eg.left_context, L});
    raw.resize(raw.size() + (size_t)rows * fdim);
    kctc::egs::cm_decompress(eg.cm.data(), raw.data() + raw.size() - (size_t)rows * fdim);
    ids.insert(ids.end(), cls.begin(), cls.end());
    for (int32_t v : cls) frames += v >= 0;
    used++;
    if ((long)ids.size() >= kBatchRows) flush();
  }
  flush();
  if (num_used) *num_used = used;
  if (num_no_ali) *num_no_ali = no_ali;
  if (num_mismatch) *num_mismatch = mismatch;
  if (num_frames) *num_frames = frames;
}

static kctc::lda::EstimateOptions options(int out_dim, double wcf, int remove_offset, double max_sv) {
  kctc::lda::EstimateOptions o;
  o.dim = out_dim;
  o.within_class_factor = wcf;
  o.remove_offset = remove_offset != 0;
  o.max_singular_value = max_sv;
  return o;
}

extern "C" {

int kctc_lda_create(kctcLda_t *out, int dim, int num_classes, int device) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(out, "kctc_lda_create: null argument");
    KCTC_REQUIRE(device >= 0, "kctc_lda_create: negative device");
    // before the handle sizes its host arrays by them
    KCTC_REQUIRE(dim >= 1 && dim <= KCTC_LDA_MAX_DIM, "lda: dim outside [1, 2048]");
    KCTC_REQUIRE(num_classes >= 1 && num_classes <= KCTC_LDA_MAX_CLASSES, "lda: num_classes outside [1, 16384]");
    *out = new kctcLda_(dim, num_classes, device);
  });
}

int kctc_lda_destroy(kctcLda_t h) {
  return kctc_guarded([&] { delete h; });
}

int kctc_lda_accumulate(kctcLda_t h, struct ihipStream_t *stream, const float *feats_dev, const int *class_dev,
                        const float *weight_dev, long R) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(h, "kctc_lda_accumulate: null handle");
    h->dev.Accumulate(stream, feats_dev, class_dev, weight_dev, R);
  });
}

int kctc_lda_get_stats(kctcLda_t h, double *zero, double *first, double *second) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(h && zero && first && second, "kctc_lda_get_stats: null argument");
    std::vector<double> z, f, s;
    h->Get(&z, &f, &s);
    std::copy(z.begin(), z.end(), zero);
    std::copy(f.begin(), f.end(), first);
    std::copy(s.begin(), s.end(), second);
  });
}

int kctc_lda_set_stats(kctcLda_t h, const double *zero, const double *first, const double *second, int add) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(h && zero && first && second, "kctc_lda_set_stats: null argument");
    h->Set(zero, first, second, add != 0);
  });
}

int kctc_lda_write(kctcLda_t h, const char *path, int binary) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(h && path, "kctc_lda_write: null argument");
    write_accs(h, path, binary != 0);
  });
}

int kctc_lda_read(kctcLda_t h, const char *path, int add) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(h && path, "kctc_lda_read: null argument");
    read_accs(h, path, add != 0);
  });
}

int kctc_lda_acc_egs(kctcLda_t h, const char *egs_rspecifier, const char *ali_rspecifier, const int *context,
                     int n_context, int blank_policy, long *num_used, long *num_no_ali, long *num_mismatch,
                     long *num_frames) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(h && egs_rspecifier && ali_rspecifier && context, "kctc_lda_acc_egs: null argument");
    acc_egs(h, egs_rspecifier, ali_rspecifier, context, n_context, blank_policy, num_used, num_no_ali, num_mismatch,
            num_frames);
  });
}

int kctc_lda_estimate(kctcLda_t h, int out_dim, double within_class_factor, int remove_offset,
                      double max_singular_value, float *M, double *cholesky) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(h && M, "kctc_lda_estimate: null argument");
    std::vector<double> z, f, s;
    h->Get(&z, &f, &s);
    kctc::lda::Estimate(z.data(), f.data(), s.data(), h->D, h->C,
                        options(out_dim, within_class_factor, remove_offset, max_singular_value), M, cholesky);
  });
}

int kctc_lda_estimate_from_stats(const double *zero, const double *first, const double *second, int dim,
                                 int num_classes, int out_dim, double within_class_factor, int remove_offset,
                                 double max_singular_value, float *M, double *cholesky) {
  return kctc_guarded([&] {
    kctc::lda::Estimate(zero, first, second, dim, num_classes,
                        options(out_dim, within_class_factor, remove_offset, max_singular_value), M, cholesky);
  });
}

int kctc_lda_test_guards(void *lda, int *intact) {
  return kctc_guarded([&] {
    KCTC_REQUIRE(lda && intact, "kctc_lda_test_guards: null argument");
    *intact = static_cast<kctcLda_t>(lda)->dev.GuardsIntact() ? 1 : 0;
  });
}

long kctc_lda_test_batch_rows(long rows) {
  const long before = g_batch_rows;
  g_batch_rows = rows > 0 ? rows : 8192;
  return before;
}

}  // extern "C"
