// call_arena.hip -- the staging arena of the batched calls (call_arena.hpp)
#include "call_arena.hpp"

namespace dsm {

int CallArena::bind(dsm_context *ctx) {
  // the context's device before the arena may grow: a thread that drives contexts on several GPUs may have another one selected
  DSM_HIP(hipSetDevice(ctx->device));
  const size_t dev_bytes = in.used + work.used + out.used, pin_bytes = in.used + out.used;
  if (dev_bytes > ctx->arena.arena_dev_bytes) {
    if (ctx->arena.arena_dev) DSM_HIP(hipFree(ctx->arena.arena_dev));
    ctx->arena.arena_dev = nullptr, ctx->arena.arena_dev_bytes = 0;
    DSM_HIP(hipMalloc(&ctx->arena.arena_dev, dev_bytes + dev_bytes / 2));
    ctx->arena.arena_dev_bytes = dev_bytes + dev_bytes / 2;
  }
  if (pin_bytes > ctx->arena.arena_pin_bytes) {
    if (ctx->arena.arena_pin) DSM_HIP(hipHostFree(ctx->arena.arena_pin));
    ctx->arena.arena_pin = nullptr, ctx->arena.arena_pin_bytes = 0;
    DSM_HIP(hipHostMalloc(&ctx->arena.arena_pin, pin_bytes + pin_bytes / 2, hipHostMallocDefault));
    ctx->arena.arena_pin_bytes = pin_bytes + pin_bytes / 2;
  }
  ctx_ = ctx, d_ = (unsigned char *)ctx->arena.arena_dev, h_ = (unsigned char *)ctx->arena.arena_pin;
  return DSM_OK;
}

int CallArena::upload(size_t bytes) const {
  DSM_HIP(hipMemcpyAsync(d_, h_, bytes, hipMemcpyHostToDevice, ctx_->stream));
  return DSM_OK;
}

int CallArena::fetch(size_t bytes) const {
  if (bytes) DSM_HIP(hipMemcpyAsync(h_ + in.used, d_ + in.used + work.used, bytes, hipMemcpyDeviceToHost, ctx_->stream));
  DSM_HIP(hipStreamSynchronize(ctx_->stream));
  return DSM_OK;
}

} // namespace dsm

void dsm_context::ArenaBuffers::release() {
  dsm::release_dev(arena_dev);
  dsm::release_pinned(arena_pin);
  arena_dev_bytes = arena_pin_bytes = 0;
}
