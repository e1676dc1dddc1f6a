// word_scan_body.h -- the body of the scan pass, as text: evt3_scan_kernel and evt2_scan_kernel include it as their whole body
// (no include guard).  It reads the kernel's parameters (sums, n_chunks, carry_in, carry_out, totals, cin) and the names Xf
// and State, and needs word_scan.h and the format's algebra.  Text and not a function, because the kernels are to keep their
// generated code: called as an inlined function template the same statements come out of the compiler scheduled differently
// (evt2_scan_kernel: 8 instructions of 1785), written into the kernel they give the code of the two separate bodies they replace.
//
// One workgroup of kScanBlock threads.  A wave owns a contiguous run of tiles of 64 chunks and walks it twice with one chunk per
// lane (consecutive lanes read and write consecutive records): first for the run's total, then, with the totals of the waves
// before it, for every chunk's incoming state and offsets.
constexpr int kScanWaves = kScanBlock / kWave;
__shared__ Xf waves[kScanWaves];
const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
State s{};  // the decoder's start state
if (carry_in) s = *carry_in;
const int64_t tiles = (n_chunks + kWave - 1) / kWave, per = (tiles + kScanWaves - 1) / kScanWaves;
const int64_t first = (int64_t)wid * per;
const int64_t lo = first < tiles ? first : tiles, hi = lo + per < tiles ? lo + per : tiles;
Xf run = identity_of<Xf>();
for (int64_t tile = lo; tile < hi; ++tile) {
  const int64_t c = tile * kWave + lane;
  const Xf inc = wave_scan_inclusive(c < n_chunks ? sums[c] : identity_of<Xf>());
  run = then(run, shfl_rec(inc, kWave - 1));
}
if (lane == 0) waves[wid] = run;
__syncthreads();  // (every thread has read *carry_in before one writes *carry_out)
Xf pre = identity_of<Xf>();
for (int w = 0; w < wid; ++w) pre = then(pre, waves[w]);
long long ev = 0, tr = 0;
apply(s, pre, ev, tr);
for (int64_t tile = lo; tile < hi; ++tile) {
  const int64_t c = tile * kWave + lane;
  const Xf inc = wave_scan_inclusive(c < n_chunks ? sums[c] : identity_of<Xf>());
  Xf exc = shfl_up_rec(inc, 1);
  if (lane == 0) exc = identity_of<Xf>();
  ChunkIn<State> in;
  in.s = s;
  in.ev = ev;
  in.tr = tr;
  apply(in.s, exc, in.ev, in.tr);
  if (c < n_chunks) cin[c] = in;
  apply(s, shfl_rec(inc, kWave - 1), ev, tr);
}
if (threadIdx.x == kScanBlock - 1) {  // (the last wave's tiles are the slab's last ones, or none: s, ev, tr are the slab's)
  *carry_out = s;
  totals[0] = ev;
  totals[1] = tr;
}
