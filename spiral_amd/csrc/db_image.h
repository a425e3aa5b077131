// The database image both servers sweep (server.cpp: n x n plaintexts, one image per shard; pack_server.cpp: 1 x 1 plaintexts, one image per
// trial, back to back): the device buffers, the form they are in, whether they hold a database, and how long they live.  Host code only.
//
// Lifetime: the image is counted.  The server that created it is its owner, the one server allowed to write it; a lane (create_lane, share_db)
// holds a reference and only sweeps.  drop() gives a reference back, the last one frees the buffers -- so destroying an owner deletes it like any
// other server, and what a lane needs of the image after that (geometry, form, epoch, loaded) it reads here.
//
// Invariant: `loaded` says that db holds a whole database in the form `format` names; `limbs`, while `limbs_valid`, holds the same database in
// limb-plane form.  Everything that writes the image goes through the calls below, which keep it:
//   - set_format: the in-place conversion.  When it fails after the first region was rewritten the image is in neither form: not loaded.
//   - a loader calls begin_rewrite() (it writes every word) or begin_partial() (it writes some: the image goes back to the packed form first)
//     before its first write and finish_load() after its last.  begin_rewrite() clears `loaded`, so a loader that fails in between leaves an image
//     that says so.  A partial loader calls dirty() where its first write is enqueued: if it fails before that, an image that was loaded still
//     is; if it fails after, the image is not loaded.
//   - update_target: where update_db_items writes, every valid form of the image (no conversion, no new epoch).
// `trk`, while on, holds the fingerprint table of the database `db` holds, whatever its form: the update calls move it with the image, set_format leaves it
// alone, and dirty() -- every loader's first write -- ends it.
#pragma once
#include "host_common.h"

namespace spiral {
namespace host {

// which kernels apply to the image and how large it is: the local first dimension (a base server's shard), 1 trial for the base server
struct DbLayout {
    bool pack;  // 1 x 1 plaintexts (the db1 kernels, sweep1_mfma_ok), else n x n (db_device_words, sweep_mfma_ok)
    uint32_t num_per, dim0, trials;
    size_t trial_words;
    static DbLayout base(uint32_t num_per, uint32_t dim0_shard) { return {false, num_per, dim0_shard, 1, db_device_words(2 * num_per, dim0_shard)}; }
    static DbLayout packed1(uint32_t num_per, uint32_t dim0, uint32_t trials) { return {true, num_per, dim0, trials, db1_device_words(num_per, dim0)}; }
    bool mfma_ok() const { return pack ? sweep1_mfma_ok(num_per, dim0) : sweep_mfma_ok(num_per, 2 * dim0); }  // the kernels can sweep the limb-plane form
    // whether an image of this layout may TAKE the limb-plane form: a SpiralPack image of 8 ciphertexts per slot (the pair form) only with option
    // pack_pair_blocks, a base image of fewer than 64 (the W forms) only with option sweep_narrow.  Asked where that is decided -- set_format(LIMBS), a
    // batch's automatic conversion (limb_view), the stage call of primitives.cpp, has_limb_form -- and nowhere else: an image that is in the form is
    // swept, updated, reloaded and converted back on mfma_ok alone, so switching an option off never strands one
    bool limbs_ok() const {
        if (!mfma_ok()) return false;
        return pack ? num_per != 8u || options().pack_pair_blocks != 0 : num_per >= 64u || options().sweep_narrow != 0;
    }
};

struct DbImage {
    DbLayout lay{};
    DevBuf db;     // trial t at db.p + t * lay.trial_words
    DevBuf limbs;  // option one_image = 0: a second image, the limb planes of a packed db (limb_view)
    bool limbs_valid = false, limbs_refused = false;  // refused: the allocation failed once, do not try again
    uint32_t format = SPIRAL_GPU_DB_PACKED;            // the form db is in
    bool loaded = false;
    uint64_t epoch = 1;  // bumped when the image is reloaded or changes form -- captured sweeps of the old form must not replay
    UpdateWork upd;      // update_db_items' workspace
    FpTrack trk;         // the tracked fingerprint (include/spiral_gpu.h "Fingerprints", Tracked): kept by the update calls, ended by every loader (dirty)
    const void* owner = nullptr;  // the server that may write the image; null once it is destroyed or has given the image up
    uint32_t refs = 1;

    // a new image of `lay`, not loaded, owned by `owner` (null: no device memory)
    static DbImage* create(const DbLayout& lay, const void* owner) {
        DbImage* img = new DbImage();
        img->lay = lay;
        img->owner = owner;
        if (img->db.alloc(lay.trial_words * lay.trials)) {
            delete img;
            return nullptr;
        }
        return img;
    }
    DbImage* share() { return refs++, this; }
    // `who` gives its reference back (the image's device current): an owner takes the right to write with it, the last reference frees the image
    static void drop(DbImage*& img, const void* who) {
        if (!img) return;
        if (img->owner == who) {
            img->owner = nullptr;
            img->upd.release();
            img->trk.release();  // (nobody is left to keep it current)
        }
        if (--img->refs == 0) {
            img->db.release();
            img->limbs.release();
            delete img;
        }
        img = nullptr;
    }
    uint32_t lanes() const { return refs - (owner ? 1u : 0u); }  // references other than the owner's
    uint64_t* trial(uint32_t t) const { return db.p + (size_t)t * lay.trial_words; }
    uint64_t device_bytes() const { return (uint64_t)(db.p ? db.words : 0) * 8u + (uint64_t)(limbs.p ? limbs.words : 0) * 8u; }

    // Converts the image between the packed form (common.h, kernels.h; the vector-ALU sweeps) and the limb planes (sweep_mfma.hip; the matrix-core
    // sweeps) IN PLACE: a slot z's region of a trial is the same byte range in both forms, so the image goes through a staging buffer of at most
    // 256 MiB a few slots at a time -- no second image, whatever the database's size.  Below 64 columns a packed tile holds pz = 64 / columns
    // slots (kernels.h db1_packed_byte: num_per columns; common.h db_tile_lane: 2 num_per columns) and it is those pz slots that share a byte range, so
    // the chunks are cut at multiples of pz.  Offline (database
    // load time or the first batch), never inside a capture.
    int set_format(uint32_t fmt, hipStream_t st) {
        if (format == fmt) return 0;
        if (fmt == SPIRAL_GPU_DB_LIMBS ? !lay.limbs_ok() : !lay.mfma_ok())
            return fail(lay.pack ? "this geometry has no limb-plane form (needs 16, 32, 64 or a power of two >= 128 ciphertexts per slot and a power-of-two first "
                                   "dimension in [128, 4096]; 8 ciphertexts per slot with option pack_pair_blocks = 1)"
                                 : "this geometry has no limb-plane form (needs >= 64 ciphertexts per slot and a power-of-two first dimension in [64, 2048]; 8, 16 or 32 "
                                   "ciphertexts per slot with option sweep_narrow = 1)");
        if (hipDeviceSynchronize() != hipSuccess) return fail("hipDeviceSynchronize failed");  // whatever reads or writes the image, on whichever stream
        const size_t per_z = lay.trial_words / kN;
        const uint32_t nic = lay.pack ? lay.num_per : 2u * lay.num_per, pz = nic < 64u ? 64u / nic : 1u;
        const uint32_t nzc = std::max(pz, (uint32_t)std::min<size_t>(kN, ((size_t)256 << 20) / (per_z * sizeof(uint64_t))) / pz * pz);
        DevBuf stage;
        if (stage.alloc(per_z * nzc)) return -1;
        const uint32_t np = lay.num_per, d = lay.pack ? lay.dim0 : 2 * lay.dim0;
        const auto convert = fmt == SPIRAL_GPU_DB_LIMBS ? (lay.pack ? launch_db1_limb_planes : launch_db_limb_planes)
                                                        : (lay.pack ? launch_db1_limb_unplanes : launch_db_limb_unplanes);
        hipError_t e = hipSuccess;
        for (uint32_t t = 0; t < lay.trials && e == hipSuccess; t++)
            for (uint32_t z = 0; z < kN && e == hipSuccess; z += nzc) {
                const uint32_t nz = std::min(nzc, kN - z);
                uint64_t* region = trial(t) + (size_t)z * per_z;
                convert(region, stage.p, np, d, st, nz);
                e = hipMemcpyAsync(region, stage.p, (size_t)nz * per_z * sizeof(uint64_t), hipMemcpyDeviceToDevice, st);
            }
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        stage.release();
        epoch++;
        limbs.release();  // (a second image from before the option was switched on)
        limbs_valid = false;
        if (e != hipSuccess) {
            loaded = false;
            format = SPIRAL_GPU_DB_PACKED;
            return fail("converting the database image failed (%s): the image is invalid, load the database again", hipGetErrorString(e));
        }
        format = fmt;
        return 0;
    }

    // the loaders' bracket (see the invariant above)
    void dirty() {
        loaded = limbs_valid = false;
        trk.release();  // a loader's writes are not followed: tracking ends
    }
    void begin_rewrite() {
        dirty();
        format = SPIRAL_GPU_DB_PACKED;
    }
    int begin_partial(hipStream_t st) {
        if (loaded) return set_format(SPIRAL_GPU_DB_PACKED, st);
        format = SPIRAL_GPU_DB_PACKED;  // (nothing to keep)
        return 0;
    }
    void finish_load() {
        loaded = true;
        limbs_valid = false;
        format = SPIRAL_GPU_DB_PACKED;
        epoch++;
    }

    // The limb-plane image for a batched sweep of n queries on the matrix cores into *out, or nullptr when that sweep does not apply (the caller's
    // threshold, the geometry); fails when it could not be built.  With the option one_image the one image changes form, in place; else a second
    // image is built from the packed one on first use (on `st`), once per database load, and refused for good when it does not fit.  The base
    // server's batches only: the pack server converts its one image (set_format).  Never call this inside a capture.
    int limb_view(uint32_t n, uint32_t threshold, hipStream_t st, const uint64_t** out) {
        *out = nullptr;
        if (format == SPIRAL_GPU_DB_LIMBS) return *out = db.p, 0;  // (whatever the threshold says: there is no other image to sweep)
        if (threshold == 0 || n < threshold || !lay.limbs_ok()) return 0;  // (either way below: the one image converted, or a second one built)
        if (options().one_image) {
            if (set_format(SPIRAL_GPU_DB_LIMBS, st)) return -1;
            return *out = db.p, 0;
        }
        if (limbs_valid) return *out = limbs.p, 0;
        if (limbs_refused) return 0;
        if (!limbs.p && limbs.alloc(db.words)) {
            // the second image does not fit beside the first (databases beyond ~120 GiB on one device): the batch sweeps in passes of two on the vector ALU
            fprintf(stderr, "spiral_gpu: no memory for the limb-plane image of the database (%zu MiB): batched sweeps stay on the vector ALU\n", (size_t)(db.words * 8 >> 20));
            (void)hipGetLastError();
            limbs_refused = true;
            return 0;
        }
        if (hipDeviceSynchronize() != hipSuccess) return fail("hipDeviceSynchronize failed");  // whatever wrote the packed image, on whichever stream
        launch_db_limb_planes(db.p, limbs.p, lay.num_per, 2 * lay.dim0, st);
        if (hipStreamSynchronize(st) != hipSuccess) return fail("building the limb-plane image failed");
        limbs_valid = true;
        return *out = limbs.p, 0;
    }

    // where update_db_items writes trial t: every form of the image that is valid now
    UpdateImage update_target(uint32_t t = 0) const {
        const size_t off = (size_t)t * lay.trial_words;
        UpdateImage u{};
        u.pack = lay.pack;
        u.num_per = lay.num_per;
        u.dim0 = lay.dim0;
        if (format == SPIRAL_GPU_DB_LIMBS) {
            u.limbs = db.p + off;
        } else {
            u.packed = db.p + off;
            if (limbs_valid) u.limbs = limbs.p + off;  // (option one_image = 0: the second image stays valid)
        }
        return u;
    }

    // what read_db_items reads of trial t: db in the form `format` names (a second image of option one_image = 0 is not looked at)
    ExportImage export_source(uint32_t t = 0) const {
        ExportImage x{};
        x.db = db.p + (size_t)t * lay.trial_words;
        x.pack = lay.pack;
        x.form = format != SPIRAL_GPU_DB_LIMBS ? DBX_PACKED : lay.pack && lay.num_per == 8u ? DBX_LIMBS8 : DBX_LIMBS;
        x.num_per = lay.num_per;
        x.dim0 = lay.dim0;
        return x;
    }
};

}  // namespace host
}  // namespace spiral
