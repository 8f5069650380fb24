// data_feed.cpp — the data layers: DataLayer (the synthetic
// stream, or an LMDB when data_param.source exists) and ImageDataLayer.  A
// RecordSource says where uint8 records come from and in which order
// (LmdbSource, ImageListSource); DataFeed is what the two share: prefetch
// thread (double buffer, the reference's BasePrefetchingDataLayer/
// BlockingQueue design collapsed to one worker + two slots,
// base_data_layer.cpp:99-134), per-image crop/mirror draw, and the uint8
// transform (transform_u8_at, math.hpp: the CPU loop here; the GPU path
// uploads the uint8 batch and runs k_transform_u8).
//
// Sharding (reference data_reader.cpp:295-301 semantics, one parser per
// rank): rank r of `world` reads record (iter*batch + j)*world + r mod N
// — ranks own disjoint record streams, deterministic and resumable from
// the solver iteration (the LMDB cursor-position analog; when N % world
// != 0 the wraparound rotates ownership across epochs, which keeps every
// record in use — the reference's full-cycle guarantee).
#include <sys/stat.h>

#include <condition_variable>
#include <fstream>
#include <mutex>
#include <thread>

#include "layers.hpp"
#include "lmdb_reader.hpp"
#include "proto_wire.hpp"

namespace camd {

struct Datum {
  int c = 0, h = 0, w = 0;
  const uint8_t* data = nullptr;
  size_t len = 0;
  long label = 0;
};

// caffe.proto Datum: channels=1 height=2 width=3 data=4 label=5
// float_data=6 encoded=7
static Datum decode_datum(const uint8_t* p, size_t n) {
  Datum d;
  wire::Reader r((const char*)p, n);
  wire::Field f;
  while (r.next(&f)) {
    switch (f.num) {
      case 1: d.c = (int)f.vint; break;
      case 2: d.h = (int)f.vint; break;
      case 3: d.w = (int)f.vint; break;
      case 4:
        d.data = (const uint8_t*)f.data;
        d.len = f.len;
        break;
      case 5: d.label = (long)f.vint; break;
      case 7:
        CHECK_(f.vint == 0) << "encoded (JPEG) Datum records are not "
                               "supported (no image codec in this build)";
        break;
      default: break;
    }
  }
  CHECK_GT_(d.c, 0);
  CHECK_(d.data != nullptr)
      << "Datum record has no uint8 `data` field (float_data Datums are "
         "not supported by this feed)";
  CHECK_EQ_((long)d.len, (long)d.c * d.h * d.w)
      << "Datum data size mismatch";
  return d;
}

// Where a feed's records come from: uint8 CHW images of one fixed shape,
// each with a label, and the order in which a rank reads them.
struct RecordSource {
  int c = 0, h = 0, w = 0;  // record dims, set by the constructor
  virtual ~RecordSource() = default;
  virtual long size() const = 0;
  // the record that sample j of batch `iter` reads
  virtual long index(uint64_t iter, int j, int batch) = 0;
  virtual void read(long idx, uint8_t* dst, float* label) = 0;
};

struct LmdbSource : RecordSource {
  LmdbReader reader;
  explicit LmdbSource(const std::string& path) {
    reader.open(path);
    CHECK_GT_(reader.size(), 0) << "empty LMDB " << path;
    auto rec0 = reader.at(0);
    Datum d0 = decode_datum(rec0.first, rec0.second);
    c = d0.c;
    h = d0.h;
    w = d0.w;
  }
  long size() const override { return reader.size(); }
  long index(uint64_t iter, int j, int batch) override {  // rank-cycle shard
    const Engine& E = Engine::get();
    return (long)((((iter * (uint64_t)batch + j) * (uint64_t)E.world) +
                   E.rank) %
                  (uint64_t)size());
  }
  void read(long idx, uint8_t* dst, float* label) override {
    auto rec = reader.at(idx);
    Datum d = decode_datum(rec.first, rec.second);
    CHECK_EQ_(d.c, c);
    CHECK_EQ_(d.h, h);
    CHECK_EQ_(d.w, w);
    memcpy(dst, d.data, d.len);
    *label = (float)d.label;
  }
};

struct DataFeed {
  std::unique_ptr<RecordSource> src;
  int dc = 0, dh = 0, dw = 0;   // record dims (src's)
  bool mirror = false;
  float scale = 1.f;
  std::vector<float> mean;       // per-channel (size dc) or per-pixel
  MeanMode mean_mode = kMeanNone;
  int batch = 0, outH = 0, outW = 0;
  Phase phase = Phase::TRAIN;

  // prefetch double buffer (uint8 batch + labels + per-image geometry)
  struct Slot {
    std::vector<uint8_t> data;   // [batch][dc][dh][dw]
    std::vector<float> labels;   // [batch]
    std::vector<int> geo;        // [batch][3] = ho, wo, mirror
    uint64_t iter = ~0ull;
    bool ready = false;
  };
  Slot slots[2];
  std::mutex mu;
  std::condition_variable cv;
  std::thread worker;
  bool stop = false;
  uint64_t want = ~0ull;     // iteration the worker should fill next
  uint64_t filling = ~0ull;  // iteration the worker is CURRENTLY filling
                             // (guards get() from racing an in-flight
                             // fill on the same slot)

  // GPU upload staging, allocated at construction in GPU mode: PINNED
  // double buffers (parity = iter & 1) so the H2D copies are truly async
  // (no pageable staging), with an event guarding reuse two
  // iterations later.  The solver thread copies slot -> pinned
  // synchronously, so the worker's vectors are free the moment get()
  // returns.
  struct Staging {
    PinnedBuf u8, geo, lab;
    GpuEvent done;  // this parity's copies have left the pinned buffers
  };
  Staging stage[2];
  // device side of the upload: the uint8 batch and its geometry (rewritten
  // every iteration) and the mean (uploaded at construction)
  DeviceBuf dev_u8, dev_geo, dev_mean;

  DataFeed(std::unique_ptr<RecordSource> source, int batch_size, Phase ph,
           const PMsgPtr& transform_param, const std::string& layer_name)
      : src(std::move(source)), dc(src->c), dh(src->h), dw(src->w),
        batch(batch_size), phase(ph) {
    setup_transform(transform_param, layer_name);
    if (Engine::get().mode == Mode::GPU) {
      const size_t usz = (size_t)batch * dc * dh * dw;
      for (Staging& st : stage) {
        st.u8.reserve(usz);
        st.geo.reserve(sizeof(int) * 3 * batch);
        st.lab.reserve(sizeof(float) * batch);
        st.done.create();
      }
      dev_u8.reserve(usz);
      dev_geo.reserve(sizeof(int) * 3 * batch);
      dev_mean.upload(mean.data(), sizeof(float) * mean.size());
    }
    worker = std::thread([this] {
      std::unique_lock<std::mutex> lk(mu);
      while (true) {
        cv.wait(lk, [this] { return stop || want != ~0ull; });
        if (stop) return;
        const uint64_t it = want;
        want = ~0ull;
        filling = it;
        Slot& s = slots[it & 1];
        lk.unlock();
        fill_slot(s, it);
        lk.lock();
        filling = ~0ull;
        cv.notify_all();
      }
    });
  }

  ~DataFeed() {
    {
      std::lock_guard<std::mutex> g(mu);
      stop = true;
    }
    cv.notify_all();
    if (worker.joinable()) worker.join();
  }

  // transform_param: crop/mirror/scale + mean_value or mean_file
  // (binaryproto, per-pixel)
  void setup_transform(const PMsgPtr& tp, const std::string& layer) {
    const int crop = tp ? (int)tp->inum("crop_size", 0) : 0;  // 0 = full
    mirror = tp && tp->boolean("mirror", false);
    scale = tp ? (float)tp->num("scale", 1.0) : 1.f;
    outH = crop > 0 ? crop : dh;
    outW = crop > 0 ? crop : dw;
    CHECK_LE_(outH, dh);
    CHECK_LE_(outW, dw);
    if (tp && tp->has("mean_file")) {
      // binaryproto BlobProto mean (full-size, subtracted in source coords)
      std::ifstream f(tp->str("mean_file"), std::ios::binary);
      CHECK_(f.good()) << "cannot read mean_file " << tp->str("mean_file");
      std::string buf((std::istreambuf_iterator<char>(f)),
                      std::istreambuf_iterator<char>());
      auto blob = wire::parse_blob(buf.data(), buf.size());
      CHECK_EQ_((long)blob.data.size(), (long)dc * dh * dw)
          << "mean_file shape mismatch";
      mean = blob.data;
      mean_mode = kMeanPerPixel;
    } else if (tp) {
      auto mv = tp->nums("mean_value");
      if (!mv.empty()) {
        // one value broadcasts, else one per channel (the reference's
        // DataTransformer check, data_transformer.cpp:203-205)
        CHECK_(mv.size() == 1 || (int)mv.size() == dc)
            << "layer '" << layer << "': " << mv.size()
            << " mean_value entries for " << dc
            << " channels (give one, or one per channel)";
        mean.resize(dc);
        for (int c = 0; c < dc; ++c)
          mean[c] = (float)mv[mv.size() == 1 ? 0 : c];
        mean_mode = kMeanPerChannel;
      }
    }
  }

  // deterministic crop/mirror stream keyed like the synthetic source
  void fill_slot(Slot& s, uint64_t iter) {
    Engine& E = Engine::get();
    const long imsz = (long)dc * dh * dw;
    s.data.resize((size_t)batch * imsz);
    s.labels.resize(batch);
    s.geo.assign((size_t)batch * 3, 0);
    const uint64_t key =
        h_splitmix64(E.seed ^ 0x17DBull ^ ((uint64_t)E.rank << 40) ^ iter);
    for (int j = 0; j < batch; ++j) {
      src->read(src->index(iter, j, batch),
                s.data.data() + (size_t)j * imsz, &s.labels[j]);
      int ho = 0, wo = 0, mir = 0;
      if (phase == Phase::TRAIN) {  // random crop + mirror (train)
        const uint64_t hj = h_splitmix64(key ^ (uint64_t)(3 * j + 1));
        const uint64_t wj = h_splitmix64(key ^ (uint64_t)(3 * j + 2));
        if (outH < dh) ho = (int)(hj % (uint64_t)(dh - outH + 1));
        if (outW < dw) wo = (int)(wj % (uint64_t)(dw - outW + 1));
        if (mirror)
          mir = (int)(h_splitmix64(key ^ (uint64_t)(3 * j + 3)) & 1);
      } else {  // center crop, no mirror (test)
        ho = (dh - outH) / 2;
        wo = (dw - outW) / 2;
      }
      s.geo[3 * j] = ho;
      s.geo[3 * j + 1] = wo;
      s.geo[3 * j + 2] = mir;
    }
    s.iter = iter;
    s.ready = true;
  }

  // get the decoded batch for `iter`: prefetched if the worker had it,
  // else decode inline; then kick the worker for iter+1
  Slot& get(uint64_t iter) {
    std::unique_lock<std::mutex> lk(mu);
    Slot& s = slots[iter & 1];
    // wait out the worker completely (assigned OR mid-fill): without the
    // `filling` guard an inline fill here could race an in-flight worker
    // fill of the SAME slot
    cv.wait(lk, [&] {
      return (want == ~0ull && filling == ~0ull) || stop;
    });
    if (!(s.ready && s.iter == iter)) {
      lk.unlock();
      fill_slot(s, iter);
      lk.lock();
    }
    s.ready = false;
    Slot& nxt = slots[(iter + 1) & 1];
    nxt.ready = false;
    want = iter + 1;
    cv.notify_all();
    return s;
  }

  // CPU transform: (uint8 - mean) * scale with crop/mirror — the
  // reference DataTransformer::Transform CPU path semantics
  void forward_cpu(uint64_t iter, const std::vector<Blob*>& top) {
    CHECK_EQ_(top[0]->num(), batch) << "data feed: top resized after setup";
    const Slot& s = get(iter);
    float* out = top[0]->mutable_cpu_data();
    const long imsz = (long)dc * dh * dw;
#pragma omp parallel for schedule(static)
    for (int j = 0; j < batch; ++j) {
      const uint8_t* im = s.data.data() + (size_t)j * imsz;
      const int* g = &s.geo[3 * j];
      float* op = out + (size_t)j * dc * outH * outW;
      for (int c = 0; c < dc; ++c)
        for (int y = 0; y < outH; ++y)
          for (int x = 0; x < outW; ++x)
            op[((long)c * outH + y) * outW + x] =
                transform_u8_at(im, c, y, x, g[0], g[1], g[2], dh, dw, outW,
                                mean.data(), mean_mode, scale);
    }
    if (top.size() > 1)
      memcpy(top[1]->mutable_cpu_data(), s.labels.data(),
             sizeof(float) * batch);
  }

  void forward_gpu(uint64_t iter, const std::vector<Blob*>& top) {
    Engine& E = Engine::get();
    Staging& st = stage[iter & 1];
    CHECK_(st.u8.p) << "data feed built in CPU mode, run in GPU mode";
    CHECK_EQ_(top[0]->num(), batch) << "data feed: top resized after setup";
    const Slot& slot = get(iter);
    const size_t usz = slot.data.size(), gsz = sizeof(int) * slot.geo.size();
    // the copies enqueued two iterations ago must have drained before the
    // pinned buffers are rewritten (GPU can run ~2 iters behind the host)
    HIP_CHECK(hipEventSynchronize(st.done.get()));
    memcpy(st.u8.p, slot.data.data(), usz);
    memcpy(st.geo.p, slot.geo.data(), gsz);
    memcpy(st.lab.p, slot.labels.data(), sizeof(float) * batch);
    HIP_CHECK(hipMemcpyAsync(dev_u8.p, st.u8.p, usz, hipMemcpyHostToDevice,
                             E.stream));
    HIP_CHECK(hipMemcpyAsync(dev_geo.p, st.geo.p, gsz, hipMemcpyHostToDevice,
                             E.stream));
    gpu::transform_u8(E.stream, dev_u8.as<uint8_t>(), batch, dc, dh, dw,
                      outH, outW, dev_geo.as<int>(), dev_mean.as<float>(),
                      mean_mode, scale, top[0]->mutable_gpu_data());
    if (top.size() > 1)
      HIP_CHECK(hipMemcpyAsync(top[1]->mutable_gpu_data(), st.lab.p,
                               sizeof(float) * batch, hipMemcpyHostToDevice,
                               E.stream));
    HIP_CHECK(hipEventRecord(st.done.get(), E.stream));
  }
};

// ---------------------------------------------------------------- Data
// hand a record source to the layer: the feed gives the top shape
static void attach_feed(DataLayer& L, std::unique_ptr<RecordSource> src) {
  L.feed_ = std::make_shared<DataFeed>(std::move(src), L.batch_, L.phase(),
                                       L.param()->sub("transform_param"),
                                       L.name());
  L.C_ = L.feed_->dc;
  L.H_ = L.feed_->outH;
  L.W_ = L.feed_->outW;
}

void DataLayer::LayerSetUp(const std::vector<Blob*>&,
                           const std::vector<Blob*>&) {
  auto dp = param_->sub("data_param");
  batch_ = dp ? (int)dp->inum("batch_size", 1) : 1;
  // LMDB source when data_param.source EXISTS on disk (reference
  // db_lmdb.cpp backend); a prototxt naming an absent dataset falls back
  // to the synthetic stream so the reference model zoo runs unmodified
  // in this dataset-less environment (round-1 drop-in contract)
  const std::string src = dp ? dp->str("source", "") : "";
  if (!src.empty()) {
    struct stat st {};
    if (stat(src.c_str(), &st) == 0) {
      attach_feed(*this, std::make_unique<LmdbSource>(src));
      return;
    }
    fprintf(stderr,
            "[caffe_amd] DataLayer '%s': source '%s' not found — using "
            "the synthetic stream\n",
            name_.c_str(), src.c_str());
  }
  auto tp = param_->sub("transform_param");
  const int crop = tp ? (int)tp->inum("crop_size", 0) : 0;
  // synthetic shape: explicit engine override, else crop_size (3 channels)
  const auto& syn = Engine::get().syn_shape;
  if (syn[1] > 0) {
    C_ = syn[0];
    H_ = syn[1];
    W_ = syn[2];
  } else if (crop > 0) {
    C_ = 3;
    H_ = W_ = crop;
  } else {
    CAMD_FATAL << "DataLayer '" << name_
               << "': no crop_size and no synthetic shape set "
                  "(caffe_set_synthetic_shape)";
  }
}

void DataLayer::Reshape(const std::vector<Blob*>&,
                        const std::vector<Blob*>& top) {
  top[0]->Reshape({batch_, C_, H_, W_});
  if (top.size() > 1) top[1]->Reshape({batch_});
}

void DataLayer::Forward_cpu(const std::vector<Blob*>&,
                            const std::vector<Blob*>& top) {
  Engine& E = Engine::get();
  if (feed_) return feed_->forward_cpu(E.data_iter, top);
  const uint64_t key = h_splitmix64(E.seed ^ ((uint64_t)E.rank << 40) ^
                                  (E.data_iter << 8));
  float* d = top[0]->mutable_cpu_data();
  const long n = top[0]->count();
  for (long i = 0; i < n; ++i)
    d[i] = h_u01(h_splitmix64(key ^ (uint64_t)i)) * 2.f - 1.f;
  if (top.size() > 1) {
    float* l = top[1]->mutable_cpu_data();
    for (long i = 0; i < batch_; ++i)
      l[i] = (float)(h_splitmix64(key ^ 0xABCDull ^ (uint64_t)i) %
                     (uint64_t)E.syn_classes);
  }
}

void DataLayer::Forward_gpu(const std::vector<Blob*>&,
                            const std::vector<Blob*>& top) {
  Engine& E = Engine::get();
  if (feed_) return feed_->forward_gpu(E.data_iter, top);
  const uint64_t key =
      h_splitmix64(E.seed ^ ((uint64_t)E.rank << 40) ^ (E.data_iter << 8));
  gpu::fill_uniform(E.stream, top[0]->count(), key, -1.f, 1.f,
                    top[0]->mutable_gpu_data());
  if (top.size() > 1)
    gpu::fill_labels(E.stream, top[1]->count(), key, E.syn_classes,
                     top[1]->mutable_gpu_data());
}

// ================================================================
// ImageData layer (reference src/caffe/layers/image_data_layer.cpp):
// image_data_param { source: listfile ("path label" per line),
// batch_size, new_height/new_width (bilinear resize), shuffle,
// root_folder } + the shared transform_param.  The image codecs are
// PPM (P6) and PGM (P5) — binary netpbm, the formats decodable without
// an image library (none exists in this environment; JPEG/PNG records
// fail with a clear message).  Like the reference, every rank reads the
// FULL list; shuffle is a per-epoch Fisher-Yates keyed by
// (seed, rank, epoch) so runs are reproducible and ranks decorrelate.
namespace {

struct PnmImage {
  int c = 0, h = 0, w = 0;
  std::vector<uint8_t> px;  // CHW
};

PnmImage load_pnm(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  CHECK_(f.good()) << "cannot open image " << path;
  std::string magic;
  f >> magic;
  CHECK_(magic == "P6" || magic == "P5")
      << "unsupported image format '" << magic << "' in " << path
      << " (only binary PPM/PGM decodable in this environment — "
         "no JPEG/PNG codec in the image)";
  auto next_int = [&]() {
    int v;
    // skip whitespace/comments (netpbm allows # comments in the header)
    while (true) {
      int ch = f.peek();
      if (ch == '#') {
        std::string line;
        std::getline(f, line);
      } else if (isspace(ch)) {
        f.get();
      } else {
        break;
      }
    }
    f >> v;
    return v;
  };
  PnmImage im;
  im.w = next_int();
  im.h = next_int();
  const int maxv = next_int();
  CHECK_EQ_(maxv, 255) << "only 8-bit netpbm supported: " << path;
  f.get();  // single whitespace before raster
  im.c = magic == "P6" ? 3 : 1;
  std::vector<uint8_t> raw((size_t)im.w * im.h * im.c);
  f.read((char*)raw.data(), (long)raw.size());
  CHECK_(f.good()) << "truncated image " << path;
  // interleaved HWC -> planar CHW (the engine/caffe layout)
  im.px.resize(raw.size());
  for (int y = 0; y < im.h; ++y)
    for (int x = 0; x < im.w; ++x)
      for (int ch = 0; ch < im.c; ++ch)
        im.px[((size_t)ch * im.h + y) * im.w + x] =
            raw[((size_t)y * im.w + x) * im.c + ch];
  return im;
}

// bilinear uint8 resize, CHW (the reference resizes via cv::resize
// INTER_LINEAR when new_height/new_width are set)
void resize_bilinear(const PnmImage& src, int nh, int nw,
                     std::vector<uint8_t>& dst) {
  dst.resize((size_t)src.c * nh * nw);
  const float sy = (float)src.h / nh, sx = (float)src.w / nw;
  for (int c = 0; c < src.c; ++c) {
    const uint8_t* sp = src.px.data() + (size_t)c * src.h * src.w;
    uint8_t* dp = dst.data() + (size_t)c * nh * nw;
    for (int y = 0; y < nh; ++y) {
      const float fy = (y + 0.5f) * sy - 0.5f;
      int y0 = (int)floorf(fy);
      const float wy = fy - y0;
      y0 = std::max(0, std::min(src.h - 1, y0));
      const int y1 = std::min(src.h - 1, y0 + 1);
      for (int x = 0; x < nw; ++x) {
        const float fx = (x + 0.5f) * sx - 0.5f;
        int x0 = (int)floorf(fx);
        const float wx = fx - x0;
        x0 = std::max(0, std::min(src.w - 1, x0));
        const int x1 = std::min(src.w - 1, x0 + 1);
        const float v =
            (1 - wy) * ((1 - wx) * sp[y0 * src.w + x0] +
                        wx * sp[y0 * src.w + x1]) +
            wy * ((1 - wx) * sp[y1 * src.w + x0] +
                  wx * sp[y1 * src.w + x1]);
        dp[y * nw + x] = (uint8_t)(v + 0.5f);
      }
    }
  }
}

struct ImageListSource : RecordSource {
  std::vector<std::pair<std::string, long>> lines;  // path, label
  bool resize = false;  // to (h, w); else every image must have that size
  bool shuffle = false;
  std::vector<long> perm;
  long perm_epoch = -1;

  ImageListSource(const std::string& list, const std::string& root, int nh,
                  int nw, bool shuffle_each_epoch)
      : resize(nh > 0 || nw > 0), shuffle(shuffle_each_epoch) {
    std::ifstream f(list);
    CHECK_(f.good()) << "cannot read image list " << list;
    std::string path;
    long label;
    while (f >> path >> label) lines.emplace_back(root + path, label);
    CHECK_GT_((long)lines.size(), 0) << "empty image list " << list;
    PnmImage first = load_pnm(lines[0].first);
    c = first.c;
    h = nh > 0 ? nh : first.h;
    w = nw > 0 ? nw : first.w;
  }
  long size() const override { return (long)lines.size(); }
  // full list per rank (reference semantics); optional keyed shuffle
  long index(uint64_t iter, int j, int batch) override {
    const uint64_t pos = iter * (uint64_t)batch + j;
    const long epoch = (long)(pos / (uint64_t)size());
    const long i = (long)(pos % (uint64_t)size());
    if (!shuffle) return i;
    if (epoch != perm_epoch) reshuffle(epoch);
    return perm[i];
  }
  void read(long idx, uint8_t* dst, float* label) override {
    const std::string& path = lines[idx].first;
    PnmImage im = load_pnm(path);
    CHECK_EQ_(im.c, c) << path;
    if (resize) {
      std::vector<uint8_t> rs;
      resize_bilinear(im, h, w, rs);
      memcpy(dst, rs.data(), rs.size());
    } else {
      CHECK_EQ_(im.h, h) << path;
      CHECK_EQ_(im.w, w) << path;
      memcpy(dst, im.px.data(), im.px.size());
    }
    *label = (float)lines[idx].second;
  }
  void reshuffle(long epoch) {
    Engine& E = Engine::get();
    const long n = size();
    perm.resize(n);
    for (long i = 0; i < n; ++i) perm[i] = i;
    uint64_t key = h_splitmix64(E.seed ^ 0x1A6Eull ^
                                ((uint64_t)E.rank << 40) ^
                                (uint64_t)epoch);
    for (long i = n - 1; i > 0; --i) {  // keyed Fisher-Yates
      key = h_splitmix64(key);
      std::swap(perm[i], perm[key % (uint64_t)(i + 1)]);
    }
    perm_epoch = epoch;
  }
};

}  // namespace

class ImageDataLayer : public DataLayer {
 public:
  using DataLayer::DataLayer;
  void LayerSetUp(const std::vector<Blob*>&,
                  const std::vector<Blob*>&) override {
    auto ip = param_->sub("image_data_param");
    CHECK_(ip) << "ImageData layer needs image_data_param";
    batch_ = (int)ip->inum("batch_size", 1);
    attach_feed(*this, std::make_unique<ImageListSource>(
                           ip->str("source"), ip->str("root_folder", ""),
                           (int)ip->inum("new_height", 0),
                           (int)ip->inum("new_width", 0),
                           ip->boolean("shuffle", false)));
  }
};

REGISTER_LAYER("ImageData", ImageDataLayer)

}  // namespace camd
