/* oc_hostio.h -- C ABI of liboc_hostio.so: everything the SB3-shaped numpy boundary returns for
 * one step, packed by ONE launch into one device buffer that crosses PCIe as one copy.
 *
 * What it replaces: the per-step obs dict -> numpy conversion a stable-baselines3 VecEnv consumer
 * sees (`VecEnv.step_wait() -> (obs dict of [n, k] arrays in the declared space dtypes, rewards,
 * dones, infos)`; reference: `DummyVecEnv` around `OvercookedMultiEnv`, trainer.py:87-121, spaces
 * gym_comm/envs/overcooked_env.py:41-85).  The stepper leaves a viewer's observation as [F][n]
 * rows; the numpy API wants [n, k] arrays of int64 / float32 / int8 per key.  `oc_pack_host`
 * gathers the rows of each dtype group, transposes, converts, and appends the float32 timestep,
 * reward, episode return, the int32 done flags and episode lengths.
 *
 * Output buffer (bytes, every block aligned to its element size because the widest come first):
 *   int64   [n][w64]     rows whose plan entry names block 0, at their column
 *   float64 [n]          ep_return   (present iff ep_return != NULL; Monitor rounds it to 6 decimals)
 *   float32 [n][w32]     block 1
 *   float32 [n]          timestep
 *   float32 [n]          reward      (present iff reward != NULL)
 *   int32   [n]          done        (present iff done != NULL)
 *   int32   [n]          ep_length   (present iff ep_length != NULL)
 *   int8    [n][w8]      block 2
 * `oc_pack_host_bytes` returns the total for the same argument presence flags.
 * plan: DEVICE int32 [F]: for observation row r, (block << 16) | column.
 * All pointers are device pointers of caller-owned tensors; nothing is synchronised, and nothing is
 * allocated except by `oc_hostio_alloc`.
 *
 * Host-mapped I/O.  `oc_hostio_alloc` is the one place where this library allocates: pinned host
 * memory, mapped into the device's address space and coherent (hipHostMalloc with the mapped and
 * coherent flags; the device-side address from hipHostGetDevicePointer), so that a kernel can read a
 * step's actions from it and write the step's packed result into it with no copy on either side.
 * `oc_pack_host_tiled` is `oc_pack_host` for an `out` that lies across PCIe: the same arguments,
 * the same bytes in the same layout, but one workgroup packs a tile of `oc_pack_host_tile()`
 * consecutive envs, lays the tile's part of every block and vector -- one contiguous span of `out`
 * each -- out in LDS and stores it 16 bytes per lane, consecutive lanes to consecutive addresses
 * (only what lies in front of a span's first 16-byte line and behind its last one is stored in
 * narrower pieces), where `oc_pack_host` stores one element per lane at a stride of a whole row.
 * Because whole spans are stored, every column of every block must be named by exactly one plan
 * entry (`oc_pack_host` leaves an unnamed column untouched).  The plan lives on the device, so of
 * this only w64 + w32 + w8 == F is verified: a plan with that sum which names one column twice and
 * another not at all is NOT detected, and the unnamed column receives unspecified bytes.  One env's
 * row of all blocks has to fit the kernel's 32 KiB of LDS (refused otherwise).  Completion is the stream's:
 * record an event behind the launch and read the host side once it has completed. */
#ifndef OC_HOSTIO_H
#define OC_HOSTIO_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#ifndef OC_API
#define OC_API __attribute__((visibility("default")))
#endif

#define OC_HOSTIO_ABI_VERSION 1

OC_API int oc_hostio_abi_version(void);
OC_API const char *oc_hostio_last_error(void);
OC_API int64_t oc_pack_host_bytes(int32_t w64, int32_t w32, int32_t w8, int32_t has_reward, int32_t has_ep_return,
                                  int32_t has_done, int32_t has_ep_length, int64_t n);
/* obs_type: element type of the rows, 0 int32, 1 int8, 2 float32 (oc_obs_cfg.obs_int8) */
OC_API int oc_pack_host(const void *obs_rows, int32_t obs_type, int32_t F, const int32_t *plan, int32_t w64,
                        int32_t w32, int32_t w8, const double *timestep, const double *reward,
                        const double *ep_return, const int32_t *done, const int32_t *ep_length, void *out,
                        int64_t n, void *stream);
/* the same call for an `out` in host-mapped memory (any device-visible `out` is valid) */
OC_API int oc_pack_host_tiled(const void *obs_rows, int32_t obs_type, int32_t F, const int32_t *plan, int32_t w64,
                              int32_t w32, int32_t w8, const double *timestep, const double *reward,
                              const double *ep_return, const int32_t *done, const int32_t *ep_length, void *out,
                              int64_t n, void *stream);
/* host only: the number of envs one workgroup of oc_pack_host_tiled packs */
OC_API int oc_pack_host_tile(void);
/* `bytes` of pinned, mapped, coherent host memory on the current device: *host for the CPU, *dev the
 * same memory for kernels.  Returns 0, or the runtime's error code with its text in
 * oc_hostio_last_error().  Free with oc_hostio_free(host) once no kernel uses it any more. */
OC_API int oc_hostio_alloc(int64_t bytes, void **host, void **dev);
OC_API int oc_hostio_free(void *host);

#ifdef __cplusplus
}
#endif
#endif
