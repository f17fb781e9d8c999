// Label encoder of the labelled data sources (dataset/dataset_lmdb.py:189-204 of the reference): the words of a batch, uploaded as packed
// code points, become the [B, max_len] target rows and the lengths the fine-tune step and the metrics consume -- on the device, like the
// crops.  Integer VALU work, one lane per cell; a few microseconds beside the input transform.
#include "common.h"

namespace {

// cell (b, t): t < n -> the class of the word's t-th code point, t == n -> eos, t > n -> padding, with n = the word's length clamped to
// [0, max_len - 1] (the host refuses longer words; the clamp keeps eos in the row whatever it is handed).  The lane of t == 0 writes lens[b].
__global__ __launch_bounds__(256) void encode_labels_kernel(const int* __restrict__ chars, const int* __restrict__ offsets,
                                                            const int* __restrict__ class_of, int eos, int padding, int unknown, int max_len,
                                                            int cells, long long* __restrict__ labels, long long* __restrict__ lens) {
  const int cell = blockIdx.x * 256 + threadIdx.x;
  if (cell >= cells) return;
  const int b = cell / max_len, t = cell - b * max_len;
  const int begin = offsets[b];
  int n = offsets[b + 1] - begin;
  n = n < 0 ? 0 : (n > max_len - 1 ? max_len - 1 : n);
  int v = padding;
  if (t < n) {
    const int c = chars[begin + t];
    const int k = (c >= 0 && c < 128) ? class_of[c] : -1;
    v = k >= 0 ? k : unknown;
  } else if (t == n) {
    v = eos;
  }
  labels[cell] = v;
  if (t == 0) lens[b] = n + 1;
}

}  // namespace

extern "C" int dig_encode_labels(const int* chars, const int* offsets, const int* class_of, int eos, int padding, int unknown, int max_len, int B,
                                 long long* labels, long long* lens, hipStream_t stream) {
  if (int rc = dig_rules::encode_labels(chars, offsets, class_of, eos, padding, unknown, max_len, B, labels, lens)) return rc;
  if (B == 0) return DIG_OK;
  const int cells = B * max_len;
  hipLaunchKernelGGL(encode_labels_kernel, dim3((cells + 255) / 256), dim3(256), 0, stream, chars, offsets, class_of, eos, padding, unknown,
                     max_len, cells, labels, lens);
  return dig_check_launch();
}
