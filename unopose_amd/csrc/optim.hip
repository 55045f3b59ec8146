// The optimiser step of the training run as three launches over ALL parameters (C ABI part 2: unopose_adam_*; unopose_amd/optim.py FusedAdam).
// What the reference does after backward() (core/unopose/engine/engine_utils.py:14-18, 53-83): torch.nan_to_num per gradient, clip_grad_norm_, then
// torch.optim.Adam -- three passes over every gradient and, with ~300 small tensors, hundreds of launches.  Here:
//   1. adam_prepare_kernel   one workgroup per CHUNK of a tensor: gradient cleaned in place (NaN -> 0, +inf -> 1e5, -inf -> -1e5; only the
//                            non-finite values are rewritten) and the chunk's sum of squares, float64, written to partials[chunk].  No atomics.
//   2. adam_finalise_kernel  one workgroup: the partials added in a fixed order -> 2-norm, clip coefficient (clip_grad_norm_'s max_norm / (norm + 1e-6),
//                            at most 1), the gate (a 1-byte device flag: "the loss was finite") and, when the gate is open, the per-tensor step
//                            counts advanced and Adam's step size lr / (1 - beta1^t) and sqrt(1 - beta2^t) written to the control block.
//   3. adam_update_kernel    over the same chunks: param, exp_avg, exp_avg_sq updated by torch.optim.Adam's rule (amsgrad = maximize = False) with
//                            the gradient times the clip coefficient (the product is NOT written back).  With the gate closed every workgroup returns
//                            at once: nothing in memory changes.
// Work is balanced over chunks, not tensors: a 3-element bias and a slice of a 1M-element weight are one workgroup each.
// Every sum has a fixed order (thread-sequential, then a tree in LDS), so two runs from equal state give equal bits.
//
// Tables (device memory, built by the caller, trusted apart from the two range checks in chunk_of()):
//   grads   n_tensors float* (the gradients are new tensors after zero_grad(set_to_none=True): refilled every step)
//   state   n_tensors x 4 pointers: param (float*), exp_avg (float*), exp_avg_sq (float*), step (int32*, one count per tensor)
//   chunks  n_chunks x {int32 tensor, int32 length (1 .. CHUNK), int64 offset (elements)}; a tensor of 0 elements has no chunk
//   block   float32: [0] norm, [1] clip coefficient, [2] gate (1.0 open / 0.0 closed), [3] unused, then per tensor [step size, sqrt(1 - beta2^t)]
#include "common.h"

namespace unopose {

constexpr int ADAM_CHUNK = 4096;  // elements per workgroup: 4 x 16-byte accesses per thread and array
constexpr int ADAM_CHUNK_WORDS = 4, ADAM_BLOCK_HEAD = 4, ADAM_BLOCK_PER_TENSOR = 2, ADAM_STATE_PTRS = 4;

struct AdamChunk {
  int tensor, length;
  long long offset;
};
static_assert(sizeof(AdamChunk) == 4 * ADAM_CHUNK_WORDS, "chunk entry layout");

// The entry of this workgroup, or length 0 when it names a tensor outside the tables / more than a chunk (a corrupt table must not leave the buffers).
__device__ __forceinline__ AdamChunk chunk_of(const AdamChunk *__restrict__ chunks, int n_tensors) {
  AdamChunk c = chunks[blockIdx.x];
  if ((unsigned)c.tensor >= (unsigned)n_tensors || c.length < 0 || c.length > ADAM_CHUNK || c.offset < 0) c.length = 0;
  return c;
}

__device__ __forceinline__ float clean_grad(float v, bool &changed) {
  if (v != v) { changed = true; return 0.f; }
  if (v == __builtin_huge_valf()) { changed = true; return 1e5f; }
  if (v == -__builtin_huge_valf()) { changed = true; return -1e5f; }
  return v;
}

// sum over the 256 threads in a fixed tree; valid in every thread
__device__ __forceinline__ double block_sum_256(double v, double *lds) {
  lds[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
    __syncthreads();
  }
  return lds[0];
}

__global__ __launch_bounds__(256) void adam_prepare_kernel(float *const *__restrict__ grads, const AdamChunk *__restrict__ chunks, int n_tensors,
                                                           double *__restrict__ partials) {
  __shared__ double lds[256];
  const AdamChunk c = chunk_of(chunks, n_tensors);
  float *g = c.length ? grads[c.tensor] + c.offset : nullptr;
  const int tid = threadIdx.x;
  double acc = 0.0;
  int done = 0;
  if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {  // 16-byte accesses for the whole quads, the last 1 .. 3 elements one by one
    const int n4 = c.length >> 2;
    for (int i = tid; i < n4; i += 256) {
      f32x4 v = reinterpret_cast<f32x4 *>(g)[i];
      bool changed = false;
      const float a = clean_grad(v[0], changed), b = clean_grad(v[1], changed), d = clean_grad(v[2], changed), e = clean_grad(v[3], changed);
      if (changed) {
        v[0] = a, v[1] = b, v[2] = d, v[3] = e;
        reinterpret_cast<f32x4 *>(g)[i] = v;
      }
      acc += (double)a * a;
      acc += (double)b * b;
      acc += (double)d * d;
      acc += (double)e * e;
    }
    done = n4 << 2;
  }
  for (int i = done + tid; i < c.length; i += 256) {
    bool changed = false;
    const float a = clean_grad(g[i], changed);
    if (changed) g[i] = a;
    acc += (double)a * a;
  }
  const double total = block_sum_256(acc, lds);
  if (tid == 0) partials[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void adam_finalise_kernel(const double *__restrict__ partials, long n_chunks, int n_tensors, void *const *__restrict__ state,
                                                            const unsigned char *__restrict__ finite, double max_norm, double lr, double beta1,
                                                            double beta2, float *__restrict__ block) {
  __shared__ double lds[256];
  double acc = 0.0;
  for (long i = threadIdx.x; i < n_chunks; i += 256) acc += partials[i];
  const double total = block_sum_256(acc, lds);
  const bool go = finite == nullptr || *finite != 0;
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(total);
    block[0] = norm;
    block[1] = max_norm >= 0.0 ? fminf((float)max_norm / (norm + 1e-6f), 1.f) : 1.f;  // clip_grad_norm_: fp32 tensors, clamp(max=1)
    block[2] = go ? 1.f : 0.f;
    block[3] = 0.f;
  }
  if (!go) return;
  for (int t = threadIdx.x; t < n_tensors; t += 256) {
    int *step = static_cast<int *>(state[(size_t)t * ADAM_STATE_PTRS + 3]);
    const int s = *step + 1;
    *step = s;
    const double bc1 = 1.0 - pow(beta1, (double)s), bc2 = 1.0 - pow(beta2, (double)s);
    block[ADAM_BLOCK_HEAD + ADAM_BLOCK_PER_TENSOR * (size_t)t] = (float)(lr / bc1);
    block[ADAM_BLOCK_HEAD + ADAM_BLOCK_PER_TENSOR * (size_t)t + 1] = (float)sqrt(bc2);
  }
}

struct AdamScalars {
  float coef, step_size, bc2_sqrt, w1, beta2, w2, eps, wd;
};

// torch.optim.adam._single_tensor_adam on one element, every operation rounded to fp32 as written (the build has -ffp-contract=off):
//   grad (+ weight_decay * param); exp_avg.lerp_(grad, 1 - beta1); exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2);
//   denom = exp_avg_sq.sqrt() / sqrt(1 - beta2^t) + eps; param.addcdiv_(exp_avg, denom, value = -step_size)
__device__ __forceinline__ void adam_element(float &p, float g, float &m, float &v, const AdamScalars &k) {
  g = g * k.coef;
  if (k.wd != 0.f) g = g + k.wd * p;
  m = m + k.w1 * (g - m);
  v = v * k.beta2 + (k.w2 * g) * g;
  const float denom = sqrtf(v) / k.bc2_sqrt + k.eps;
  p = p - k.step_size * (m / denom);
}

__global__ __launch_bounds__(256) void adam_update_kernel(const float *const *__restrict__ grads, void *const *__restrict__ state,
                                                          const AdamChunk *__restrict__ chunks, int n_tensors, const float *__restrict__ block,
                                                          float w1, float beta2, float w2, float eps, float wd) {
  if (block[2] == 0.f) return;  // gate closed: nothing is read or written
  const AdamChunk c = chunk_of(chunks, n_tensors);
  if (c.length == 0) return;
  const float *g = grads[c.tensor] + c.offset;
  void *const *st = state + (size_t)c.tensor * ADAM_STATE_PTRS;
  float *p = static_cast<float *>(st[0]) + c.offset, *m = static_cast<float *>(st[1]) + c.offset, *v = static_cast<float *>(st[2]) + c.offset;
  const AdamScalars k = {block[1], block[ADAM_BLOCK_HEAD + ADAM_BLOCK_PER_TENSOR * (size_t)c.tensor],
                         block[ADAM_BLOCK_HEAD + ADAM_BLOCK_PER_TENSOR * (size_t)c.tensor + 1], w1, beta2, w2, eps, wd};
  const int tid = threadIdx.x;
  int done = 0;
  if (((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) & 15) == 0) {
    const int n4 = c.length >> 2;
    for (int i = tid; i < n4; i += 256) {
      const f32x4 g4 = reinterpret_cast<const f32x4 *>(g)[i];
      f32x4 p4 = reinterpret_cast<f32x4 *>(p)[i], m4 = reinterpret_cast<f32x4 *>(m)[i], v4 = reinterpret_cast<f32x4 *>(v)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = p4[e], me = m4[e], ve = v4[e];
        adam_element(pe, g4[e], me, ve, k);
        p4[e] = pe, m4[e] = me, v4[e] = ve;
      }
      reinterpret_cast<f32x4 *>(p)[i] = p4;
      reinterpret_cast<f32x4 *>(m)[i] = m4;
      reinterpret_cast<f32x4 *>(v)[i] = v4;
    }
    done = n4 << 2;
  }
  for (int i = done + tid; i < c.length; i += 256) adam_element(p[i], g[i], m[i], v[i], k);
}

}  // namespace unopose

using namespace unopose;

extern "C" {

int unopose_adam_table_ints(int what) {
  switch (what) {
    case 0: return ADAM_CHUNK;
    case 1: return ADAM_CHUNK_WORDS;
    case 2: return ADAM_BLOCK_HEAD;
    case 3: return ADAM_BLOCK_PER_TENSOR;
    case 4: return ADAM_STATE_PTRS;
  }
  return -1;
}

int unopose_adam_prepare(const void *grads_dev, const void *chunks_dev, long n_chunks, int n_tensors, double *partials, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(n_chunks >= 0 && n_chunks <= 0x7FFFFFFFL && n_tensors >= 0, "adam_prepare: bad sizes (%ld chunks, %d tensors)", n_chunks, n_tensors);
  if (n_chunks == 0) return UNOPOSE_OK;
  UNOPOSE_REQUIRE(grads_dev && chunks_dev && partials && n_tensors > 0, "adam_prepare: null pointer");
  hipLaunchKernelGGL(adam_prepare_kernel, dim3((unsigned)n_chunks), dim3(256), 0, (hipStream_t)stream, (float *const *)grads_dev,
                     (const AdamChunk *)chunks_dev, n_tensors, partials);
  return check_launch("adam_prepare");
}

int unopose_adam_finalise(const double *partials, long n_chunks, int n_tensors, const void *state_dev, const void *finite, double max_norm, double lr,
                          double beta1, double beta2, float *block, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(n_chunks >= 0 && n_chunks <= 0x7FFFFFFFL && n_tensors >= 0, "adam_finalise: bad sizes (%ld chunks, %d tensors)", n_chunks, n_tensors);
  UNOPOSE_REQUIRE(block && (n_chunks == 0 || partials) && (n_tensors == 0 || state_dev), "adam_finalise: null pointer");
  UNOPOSE_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "adam_finalise: betas (%g, %g) outside [0, 1)", beta1, beta2);
  hipLaunchKernelGGL(adam_finalise_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, n_chunks, n_tensors, (void *const *)state_dev,
                     (const unsigned char *)finite, max_norm, lr, beta1, beta2, block);
  return check_launch("adam_finalise");
}

int unopose_adam_update(const void *grads_dev, const void *state_dev, const void *chunks_dev, long n_chunks, int n_tensors, const float *block,
                        double beta1, double beta2, double eps, double weight_decay, unopose_stream_t stream) {
  UNOPOSE_REQUIRE(n_chunks >= 0 && n_chunks <= 0x7FFFFFFFL && n_tensors >= 0, "adam_update: bad sizes (%ld chunks, %d tensors)", n_chunks, n_tensors);
  if (n_chunks == 0) return UNOPOSE_OK;
  UNOPOSE_REQUIRE(grads_dev && state_dev && chunks_dev && block && n_tensors > 0, "adam_update: null pointer");
  hipLaunchKernelGGL(adam_update_kernel, dim3((unsigned)n_chunks), dim3(256), 0, (hipStream_t)stream, (const float *const *)grads_dev,
                     (void *const *)state_dev, (const AdamChunk *)chunks_dev, n_tensors, block, (float)(1.0 - beta1), (float)beta2,
                     (float)(1.0 - beta2), (float)eps, (float)weight_decay);
  return check_launch("adam_update");
}

}  // extern "C"
