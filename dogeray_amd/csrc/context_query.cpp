// What the queries on caller lists share (dr_trace_rays, dr_trace_radiance, dr_query_nearest, dr_trace_all_hits): a list of n items goes to the device and
// its channels come back, or -- device_pointers -- the kernels read and write the caller's memory.  Everything here is enqueued on c->stream, in the order
// the entry point calls it: query_begin, [query_scratch], [query_cursor], the entry point's launches, query_end.
#include "context.hpp"

namespace dr {

// the slot -> object map on the device, for the kernels that write `object`: uploaded once per scene (dr_context_upload releases the old one)
int ensure_slot_to_orig(dr_context* c) {
  if (c->slot_to_orig_dev) return DR_OK;
  DR_TRY(c->slot_to_orig_dev.alloc(c->slot_to_orig.size()));
  if (!c->slot_to_orig.empty())
    HIP_TRY(hipMemcpyAsync(c->slot_to_orig_dev, c->slot_to_orig.data(), c->slot_to_orig.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  return DR_OK;
}

// Fills io with the device addresses of the inputs and of the wanted channels of n > 0 items; an entry of a channel is an item (per_item) or one of an
// item's K.  Host pointers: staging holds every input, given or not, in the order of `in`, then the wanted channels in the order of `out`; the given
// inputs are copied in.  Staging is aligned as hipMalloc aligns and every offset is a multiple of 4 bytes only (a channel of bytes is padded to one),
// so AN INPUT OF 8-BYTE ELEMENTS GOES FIRST (dr_trace_radiance's seeds): at offset 0 it is aligned whatever n is.  The accumulator's stages
// (context_accum.cpp) come here with their pixels as the items and no input: the wanted outputs are carved and downloaded as a query's channels are.
int query_begin(dr_context* c, size_t n, size_t K, const QueryIn* in, int n_in, const QueryOut* out, int n_out, bool device_pointers, QueryIo& io) {
  memset(&io, 0, sizeof(io));
  size_t bytes = 0;
  for (int k = 0; k < n_in; k++) bytes += n * (size_t)in[k].words * 4;
  for (int k = 0; k < n_out; k++) {
    io.out_bytes[k] = (out[k].per_item ? n : n * K) * (size_t)out[k].words * (size_t)out[k].unit;
    if (out[k].p) bytes += (io.out_bytes[k] + 3) & ~(size_t)3;
  }
  if (device_pointers) {
    for (int k = 0; k < n_in; k++) io.in[k] = in[k].p;
    for (int k = 0; k < n_out; k++) io.out[k] = out[k].p;
    return DR_OK;
  }
  DR_TRY(c->query_staging.grow(bytes, c->stream));
  size_t off = 0;
  for (int k = 0; k < n_in; k++) {
    const size_t size = n * (size_t)in[k].words * 4;
    if (in[k].p) {
      HIP_TRY(hipMemcpyAsync(c->query_staging + off, in[k].p, size, hipMemcpyHostToDevice, c->stream));
      io.in[k] = c->query_staging + off;
    }
    off += size;
  }
  for (int k = 0; k < n_out; k++)
    if (out[k].p) { io.out[k] = c->query_staging + off; off += (io.out_bytes[k] + 3) & ~(size_t)3; }
  return DR_OK;
}

// the two words per entry between a walk kernel and the pass behind it
int query_scratch(dr_context* c, size_t entries, uint32_t*& words) {
  DR_TRY(c->query_scratch.grow(2 * entries, c->stream));
  words = c->query_scratch;
  return DR_OK;
}

// a persistent kernel's cursor into the list, zeroed for this launch: a stale cursor would drop rays
int query_cursor(dr_context* c, unsigned*& cursor) {
  if (!c->query_cursor) DR_TRY(c->query_cursor.alloc(1));
  HIP_TRY(hipMemsetAsync(c->query_cursor, 0, sizeof(unsigned), c->stream));
  cursor = c->query_cursor;
  return DR_OK;
}

// behind the launches.  Host pointers: the wanted channels are copied out and the call waits for them; device pointers: the work stays queued
int query_end(dr_context* c, const QueryOut* out, int n_out, bool device_pointers, const QueryIo& io) {
  if (device_pointers) return DR_OK;
  for (int k = 0; k < n_out; k++)
    if (out[k].p) HIP_TRY(hipMemcpyAsync(out[k].p, io.out[k], io.out_bytes[k], hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return DR_OK;
}

}  // namespace dr
