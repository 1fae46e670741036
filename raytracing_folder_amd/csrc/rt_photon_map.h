// rt_photon_map.h -- the global photon map of a scene: whose it is and where it lies.  rt_scene (rt_host.h) holds exactly one
// GlobalPhotons and nobody learns where the map is but through it; rt_photons.cpp is the file that works on it.  Nothing of HIP
// here (a device is an address): tests/photon_map_states.cpp compiles this header alone and walks every transition.
#pragma once
#include <cassert>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/rt_mi355x.h"

struct DeviceState;

// A map handed over with rt_scene_set_photons is the CALLER's: balanced, in SceneData::photons, and it stays through scene edits.
// A map made by the photon pass (rt_scene_generate_photons, rt_render_begin) is GENERATED, that is DERIVED from the scene: whatever
// it was traced through (nodes, meshes, materials, lights, another XML) changing drops it, and rt_render_begin makes a new one when
// there is none or when the render asks for another count / bounce limit / seed -- the reference runs generatePhotonMap() on every
// BeginRender (FIN/main.cpp:984-990).  It is kept as generatePhotonMap leaves it BEFORE balancing (1-based, [0] zero) together
// with the 1-based indices of the few photons LocatePhotons could not reach after balancing (rt::UnreachablePhotons), and it STAYS
// on the device that generated it (DeviceState::raw_photons) until somebody needs it on the host: the .dat dump,
// rt_scene_get_photons, another device, a later photon pass on that device.  Its balanced form (`balanced` below: the scene's
// SceneData::photons) is produced only when somebody asks for it.
//
// INVARIANT: a generated map has a host raw copy (n + 1 records) or a device residence, or both; a map that is not generated has
// neither, and no skip list; no map at all has n == 0.
class GlobalPhotons {
public:
    struct Params { uint32_t count; int bounce; uint32_t seed; };
    // the unbalanced photons where they lie on a device (1-based, n of them); photons == NULL: not there
    struct DeviceSource { const rt_photon *photons = nullptr; uint32_t n = 0; explicit operator bool() const { return photons != nullptr; } };

    uint32_t count() const { return n_; }
    bool is_generated() const { return owner_ == GENERATED; }
    // whether a render with these photon parameters can use the map: a generated one serves only what it was generated with
    bool serves(uint32_t count, int bounce, uint32_t seed) const
    {
        return n_ != 0 && (owner_ != GENERATED || (params_.count == count && params_.bounce == bounce && params_.seed == seed));
    }
    const std::vector<uint32_t> &skip() const { return skip_; }
    const std::vector<rt_photon> &host_raw() const { return raw_; }
    bool host_copy_missing() const { return owner_ == GENERATED && raw_.empty(); }
    DeviceState *device() const { return dev_; }
    DeviceSource source_on(const DeviceState *D) const { return D && D == dev_ ? DeviceSource{dev_photons_, n_} : DeviceSource{}; }
    bool invariant() const
    {
        if (owner_ == GENERATED) return (!raw_.empty() || dev_) && (raw_.empty() || raw_.size() == (size_t)n_ + 1) && (dev_ != nullptr) == (dev_photons_ != nullptr);
        return raw_.empty() && skip_.empty() && !dev_ && !dev_photons_ && (owner_ == CALLER) == (n_ != 0);
    }

    // rt_scene_set_photons: the caller's balanced map (n == 0: none) replaces whatever there was
    void set_callers(std::vector<rt_photon> &balanced, const rt_photon *photons, uint32_t n)
    {
        clear();
        if (n == 0) balanced.clear();
        else balanced.assign(photons, photons + (size_t)n + 1);
        owner_ = n ? CALLER : NONE; n_ = n;
        assert(invariant());
    }
    // the map the photon pass just left in dev_photons (D's raw_photons): `raw` is its host copy if one was made, else empty
    void adopt_generated(std::vector<rt_photon> &balanced, DeviceState *D, const rt_photon *dev_photons, uint32_t n, Params params,
                         std::vector<uint32_t> &&skip, std::vector<rt_photon> &&raw)
    {
        assert(D && dev_photons);
        balanced.clear();
        owner_ = GENERATED; n_ = n; params_ = params;
        skip_ = std::move(skip); raw_ = std::move(raw);
        dev_ = D; dev_photons_ = dev_photons;
        assert(invariant());
    }
    // a generated map with the balanced form derived from it; true when there was one (the caller's stays)
    bool drop_generated(std::vector<rt_photon> &balanced)
    {
        if (owner_ != GENERATED) return false;
        clear();
        balanced.clear();
        assert(invariant());
        return true;
    }
    void set_host_copy(std::vector<rt_photon> &&raw)
    {
        assert(owner_ == GENERATED && raw.size() == (size_t)n_ + 1);
        raw_ = std::move(raw);
        assert(invariant());
    }
    // D's buffer is about to hold something else.  A map that lives only there must have come to the host first (leaving_device
    // in rt_photons.cpp sees to it); after this, source_on(D) answers nothing.
    void leave_device(const DeviceState *D)
    {
        if (D != dev_) return;
        assert(!raw_.empty());
        dev_ = nullptr; dev_photons_ = nullptr;
        assert(invariant());
    }

private:
    enum Owner { NONE, CALLER, GENERATED };
    void clear() { owner_ = NONE; n_ = 0; params_ = Params{}; skip_.clear(); raw_.clear(); dev_ = nullptr; dev_photons_ = nullptr; }
    Owner owner_ = NONE;
    uint32_t n_ = 0;                            // photons of the map, whoever owns it
    Params params_{};                           // generated: what it was generated with
    std::vector<uint32_t> skip_;                // generated: 1-based raw indices balancing would put out of LocatePhotons' reach
    std::vector<rt_photon> raw_;                // generated: the unbalanced host copy, or empty
    DeviceState *dev_ = nullptr;                // generated: the device it still lies on, with the buffer there; NULL: on none
    const rt_photon *dev_photons_ = nullptr;
};
