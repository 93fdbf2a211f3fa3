// Package hip is the MI355X backend of the path tracer: a drop-in for package
// internal/engine/gpu (the OpenGL backend) behind engine.RenderInto.
//
//	gpu.Render(sc *scene.Scene, cfg gpu.RenderConfig, img *image.RGBA, progress func()) error
//
// has the same signature here.  The scene is flattened into the plain C structs of
// include/ptcore.h and rendered by libptcore.so (HIP kernels for gfx950).
//
// NOT COMPILED IN THE BUILD IMAGE: no Go toolchain exists there.  The file is the binding a
// maintainer adds to the reference tree (see INTEGRATION.md); it uses only documented cgo rules
// (no Go pointers retained by C, img.Pix is pointer-free and may be passed directly).
package hip

/*
#cgo CFLAGS: -I${SRCDIR}/../../../../include
#cgo LDFLAGS: -L${SRCDIR}/../../../../path_trace_golang_amd -lptcore -Wl,-rpath,${SRCDIR}/../../../../path_trace_golang_amd
#include <stdlib.h>
#include "ptcore.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"image"
	"math"
	"os"
	"reflect"
	"runtime"
	"strconv"
	"strings"
	"sync"
	"unsafe"

	"github.com/user/pathtracer/internal/scene"
)

// RenderConfig mirrors gpu.RenderConfig (internal/engine/gpu/gpu.go:227-232).
type RenderConfig struct {
	Width        int
	Height       int
	SamplesPerPx int
	MaxDepth     int
}

var (
	mu      sync.Mutex // one render at a time, like the reference's single GL worker (gpu.go:2534-2546)
	ctx     *C.pt_ctx
	initErr error // sticky, like gpu.go:279-286
	devices = 1
	seed    = uint64(1)

	noiseSet    bool // false: PATHTRACER_GPU_NOISE / PATHTRACER_GPU_NOISE_STEP decide
	noiseTarget float64
	noiseStep   = 16
	lastSpp     int     // samples per pixel of the last frame Render finished
	lastNoise   float64 // its frame noise (0 without a noise target)

	adaptiveSet    bool // false: PATHTRACER_GPU_ADAPTIVE / PATHTRACER_GPU_ADAPTIVE_MIN_SPP decide
	adaptiveOn     bool
	adaptiveMinSpp int
	lastAdaptive   AdaptiveState // pt_adaptive_state of the last frame (zero unless it was adaptive)

	atrousSet    bool // false: PATHTRACER_GPU_ATROUS / PATHTRACER_GPU_ATROUS_ITERS decide
	atrousOn     bool
	atrousIters  = 5
	featuresK    = -1        // -1: not said, PATHTRACER_GPU_FEATURES decides (and without it: 4 under the filter where the scene allows)
	lastAtrous   AtrousStats // pt_atrous_stats of the last frame (zero unless it was filtered)
	temporalSet  bool        // false: PATHTRACER_GPU_TEMPORAL decides
	temporalOn   bool
	lastTemporal TemporalStats // pt_temporal_stats of the last frame (zero unless it was accumulated)
	clipSet      bool          // false: PATHTRACER_GPU_TEMPORAL_CLIP decides
	clipGamma    float64
	motionSet    bool // false: PATHTRACER_GPU_TEMPORAL_MOTION decides
	motionOn     bool
	idsOn        bool           // pt_set_object_ids(1) was the last thing said to the context
	walkSet      bool           // false: PATHTRACER_GPU_FEATURE_WALK decides
	walkWanted   bool
	walkOn       bool           // pt_set_feature_walk(1) was the last thing said to the context
	fogWalkSet    bool          // false: PATHTRACER_GPU_FOG_WALK decides
	fogWalkWanted bool
	fogWalkOn     bool          // pt_set_fog_walk(1) was the last thing said to the context
	shadingWalkSet    bool      // false: PATHTRACER_GPU_SHADING_WALK decides
	shadingWalkWanted bool
	shadingWalkOn     bool      // pt_set_shading_walk(1) was the last thing said to the context
	shadingFeaturesSet    bool  // false: PATHTRACER_GPU_SHADING_FEATURES decides
	shadingFeaturesWanted bool
	shadingFeaturesOn     bool  // pt_set_shading_features(1) was the last thing said to the context
	refitSet     bool           // false: PATHTRACER_GPU_BVH_REFIT decides
	refitWanted  float64
	refitSaid    float64        // the bound pt_set_bvh_refit was last given (0: never said, or off)
	buildSet     bool           // false: PATHTRACER_GPU_BVH_BUILD decides
	buildWanted  bool
	buildSaid    bool           // pt_set_bvh_build(1) was the last thing said to the context
	accumulated  *scene.Scene   // a copy of the scene of the last frame accumulated with displaced reprojection on (nil: none)
	lastMotion   TemporalMotion // pt_temporal_motion_stats of the last frame (zero unless it was accumulated with the rule on)

	filteredSet    bool        // false: PATHTRACER_GPU_FILTERED_NOISE decides
	filteredTarget float64     // the noise target on the filtered frame (0 = off)
	lastHalves     HalvesStats // pt_halves_stats of the last check of the last frame (zero unless that stop rule was in force)

	filteredAdaptiveSet    bool // false: PATHTRACER_GPU_FILTERED_ADAPTIVE and PATHTRACER_GPU_POOL decide
	filteredAdaptiveTarget float64
	filteredAdaptivePool   = 1
	filteredAdaptiveOn     bool // pt_set_adaptive_filtered is in force on ctx (said only where it was ever on)
)

// HalvesStats mirrors pt_halves_stats: the measured and the propagated noise of the filtered frame at the last check.
type HalvesStats struct {
	Ms         float64
	Launches   int
	Iterations int
	Noise      float64 // measured: the two halves' difference
	NoiseModel float64 // propagated: optimistic
	BadPixels  uint64
	SppMin     int
}

// AtrousStats mirrors pt_atrous_stats: what the a-trous filter did to the last frame.
type AtrousStats struct {
	Ms          float64
	Launches    int
	Iterations  int
	NoiseBefore float64
	NoiseAfter  float64
	BadPixels   uint64
	Features    int // feature samples per pixel the frame collected
}

// AdaptiveState mirrors struct pt_adaptive_state: the block table of an adaptive frame.
type AdaptiveState struct {
	Blocks, ActiveBlocks, Samples uint64
	SppMin, SppMax                int
	WorstActive                   float64
}

// SetDevices selects how many GPUs (ordinals 0..n-1) the frame is tiled over.
// The tiles of a frame are collected on device 0 by peer copies over xGMI, or -- with
// PTCORE_GATHER=rccl in the environment when the context is created -- by grouped RCCL
// send / receive (libptcore loads librccl.so itself in that case; nothing to link here).
func SetDevices(n int) {
	mu.Lock()
	defer mu.Unlock()
	if ctx != nil {
		C.pt_destroy(ctx)
		ctx = nil
		idsOn, accumulated = false, nil
		walkOn = false
		fogWalkOn = false
		shadingWalkOn = false
		shadingFeaturesOn = false
		refitSaid = 0
		buildSaid = false
	}
	initErr = nil
	if n > 0 {
		devices = n
	}
}

// SetSeed selects the sample streams (the CPU engine seeds from the clock, random.go:14-16).
func SetSeed(s uint64) { seed = s }

// SetNoiseTarget makes Render stop at the first check where the frame noise (pt_noise_estimate, DESIGN 3.9) is at or below
// target, checking every step samples per pixel, with cfg.SamplesPerPx as the cap.  target <= 0 turns the rule off.
func SetNoiseTarget(target float64, step int) {
	mu.Lock()
	defer mu.Unlock()
	noiseSet = true
	noiseTarget = target
	if step >= 1 {
		noiseStep = step
	} else {
		noiseStep = 16
	}
}

// SetAdaptive makes the noise target the target of every 8x8 block (pt_set_adaptive, DESIGN 3.10): blocks stop one by one and
// each pixel keeps the samples its block got; minSpp samples every block gets before the first check.  It takes effect together
// with a noise target.
func SetAdaptive(on bool, minSpp int) {
	mu.Lock()
	defer mu.Unlock()
	adaptiveSet, adaptiveOn = true, on
	if minSpp < 0 {
		minSpp = 0
	}
	adaptiveMinSpp = minSpp
}

// SetAtrous makes Render write the variance-guided a-trous filtered image (pt_atrous, DESIGN 3.11) instead of the plain finish:
// moments are collected, and the first-hit feature planes too where the scene allows them.  iterations is 0..6.
func SetAtrous(on bool, iterations int) {
	mu.Lock()
	defer mu.Unlock()
	atrousSet, atrousOn = true, on
	if iterations < 0 || iterations > 6 {
		iterations = 5
	}
	atrousIters = iterations
}

// SetFilteredNoise puts the noise target on the filtered frame (DESIGN 3.12): with the filter on (SetAtrous) the frame collects the
// half-buffer sums (pt_set_halves), samples are added a noise step at a time (SetNoiseTarget's step, or PATHTRACER_GPU_NOISE_STEP),
// after every step with at least 4 samples done pt_atrous_halves runs with the filter's configuration, and the frame stops at the
// first check whose measured noise is at or below target, cfg.SamplesPerPx being the cap.  The image is pt_atrous on the full sums.
// target <= 0 turns the rule off.  It is ignored without the filter and is an error beside a frame noise target or GL shading.
func SetFilteredNoise(target float64) {
	mu.Lock()
	defer mu.Unlock()
	filteredSet = true
	if target < 0 {
		target = 0
	}
	filteredTarget = target
}

// LastHalves reports the figures of the last check of the last frame Render finished under SetFilteredNoise.
func LastHalves() HalvesStats {
	mu.Lock()
	defer mu.Unlock()
	return lastHalves
}

// filteredRule: the noise target on the filtered frame in force (SetFilteredNoise, else the environment; 0 = off, also without the filter).
func filteredRule() float64 {
	if on, _ := atrousRule(); !on {
		return 0
	}
	if filteredSet {
		return filteredTarget
	}
	if v, err := strconv.ParseFloat(strings.TrimSpace(os.Getenv("PATHTRACER_GPU_FILTERED_NOISE")), 64); err == nil && v > 0 && !math.IsInf(v, 0) {
		return v
	}
	return 0
}

// SetFilteredAdaptive makes the frame adaptive with the blocks stopped by the filtered frame's pooled noise (pt_set_adaptive_filtered,
// DESIGN 3.12a): with the filter on (SetAtrous), every 8x8 block stops once the noise measured in the filtered frame over the blocks
// within pool blocks (0..4, anything else counts as 1) of it is at or below target; the step and minSpp are SetNoiseTarget's and
// SetAdaptive's.  target <= 0 turns the rule off.  It is ignored without the filter and is an error beside a frame noise target, the
// filtered noise target or GL shading.  Not set: PATHTRACER_GPU_FILTERED_ADAPTIVE and PATHTRACER_GPU_POOL decide.
func SetFilteredAdaptive(target float64, pool int) {
	mu.Lock()
	defer mu.Unlock()
	filteredAdaptiveSet = true
	if target < 0 {
		target = 0
	}
	if pool < 0 || pool > 4 {
		pool = 1
	}
	filteredAdaptiveTarget, filteredAdaptivePool = target, pool
}

// filteredAdaptiveRule: the block target on the filtered frame's pooled noise in force and the pool radius (0 = off, also without the filter).
func filteredAdaptiveRule() (float64, int) {
	if on, _ := atrousRule(); !on {
		return 0, 1
	}
	if filteredAdaptiveSet {
		return filteredAdaptiveTarget, filteredAdaptivePool
	}
	pool := 1
	if v, err := strconv.Atoi(strings.TrimSpace(os.Getenv("PATHTRACER_GPU_POOL"))); err == nil && v >= 0 && v <= 4 {
		pool = v
	}
	if v, err := strconv.ParseFloat(strings.TrimSpace(os.Getenv("PATHTRACER_GPU_FILTERED_ADAPTIVE")), 64); err == nil && v > 0 && !math.IsInf(v, 0) {
		return v, pool
	}
	return 0, pool
}

// ReadBlockFigures reads pt_read_block_figures of the last frame rendered under SetFilteredAdaptive: the last deciding check's pooled
// figure and the block's own, row-major over the grid of ((width + 7) / 8) x ((height + 7) / 8) blocks, and the checks that decided.
func ReadBlockFigures(width, height int) (pooled, own []float64, checks int, err error) {
	mu.Lock()
	defer mu.Unlock()
	if ctx == nil {
		return nil, nil, 0, errors.New("pt_read_block_figures: no context yet")
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	n := ((width + 7) / 8) * ((height + 7) / 8)
	if n <= 0 {
		return nil, nil, 0, errors.New("pt_read_block_figures: empty frame")
	}
	pooled, own = make([]float64, n), make([]float64, n)
	var c C.int32_t
	if rc := C.pt_read_block_figures(ctx, (*C.double)(unsafe.Pointer(&pooled[0])), (*C.double)(unsafe.Pointer(&own[0])), &c); rc != C.PT_OK {
		return nil, nil, 0, lastError("pt_read_block_figures")
	}
	return pooled, own, int(c), nil
}

// TemporalStats mirrors pt_temporal_stats: what the temporal accumulation did to the last frame.
type TemporalStats struct {
	Ms                                   float64
	Launches, Iterations                 int
	Reprojected, Disoccluded, BadPixels  uint64
	MeanLen                              float64
	NoiseBefore, NoiseBlended, NoiseAfter float64
}

// SetTemporal turns the temporal accumulation on (pt_temporal, DESIGN 3.13), for a caller that renders frame after frame while the
// camera moves: the context of this package keeps a history from Render to Render, and Render's image is the frame blended into the
// reprojected history, then filtered, in place of pt_atrous's.  On brings the moments, the filter and 4 feature samples per pixel with
// it (unless SetFeatures / PATHTRACER_GPU_FEATURES name another number).  Change cfg.Seed from frame to frame -- the blended variance
// assumes independent frames -- and call ResetTemporal after a scene edit or a cut.  Not set: PATHTRACER_GPU_TEMPORAL decides.
func SetTemporal(on bool) {
	mu.Lock()
	defer mu.Unlock()
	temporalSet, temporalOn = true, on
}

// Temporal reports whether the accumulation is in force.
func Temporal() bool {
	mu.Lock()
	defer mu.Unlock()
	return temporalRule()
}

// ResetTemporal empties the history (pt_temporal_reset).
func ResetTemporal() error {
	mu.Lock()
	defer mu.Unlock()
	if ctx == nil {
		return nil
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	accumulated = nil
	if rc := C.pt_temporal_reset(ctx); rc != C.PT_OK {
		return lastError("pt_temporal_reset")
	}
	return nil
}

// LastTemporal reports the accumulation's figures for the last frame Render finished (the zero value unless it was accumulated).
func LastTemporal() TemporalStats {
	mu.Lock()
	defer mu.Unlock()
	return lastTemporal
}

// TemporalClip mirrors struct pt_temporal_clip_stats: the history clip of the last accumulated frame.
type TemporalClip struct {
	Gamma                float64
	Clipped, Reprojected uint64
}

// SetTemporalClip sets the history clip of the accumulation (pt_temporal_set_clip, DESIGN 3.13a): before the blend the reprojected
// history is clamped to the frame's mean +- gamma * sqrt(var_frame + var_history).  0 = off (the default); 2.5 is the recommended
// value; a NaN, a negative or an infinite gamma is taken as 0.  Read by Render when the accumulation is on.  Not set:
// PATHTRACER_GPU_TEMPORAL_CLIP decides.
func SetTemporalClip(gamma float64) {
	mu.Lock()
	defer mu.Unlock()
	if math.IsNaN(gamma) || math.IsInf(gamma, 0) || gamma < 0 {
		gamma = 0
	}
	clipSet, clipGamma = true, gamma
}

// TemporalClipStats reports pt_temporal_clip_stats of the package's context: the gamma, the clipped and the reprojected pixels of
// the last accumulated frame.  An error while the history is empty.
func TemporalClipStats() (TemporalClip, error) {
	mu.Lock()
	defer mu.Unlock()
	if ctx == nil {
		return TemporalClip{}, errors.New("pt_temporal_clip_stats: no context yet")
	}
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	var cs C.struct_pt_temporal_clip_stats
	if rc := C.pt_temporal_clip_stats(ctx, &cs); rc != C.PT_OK {
		return TemporalClip{}, lastError("pt_temporal_clip_stats")
	}
	return TemporalClip{Gamma: float64(cs.gamma), Clipped: uint64(cs.clipped), Reprojected: uint64(cs.reprojected)}, nil
}

// TemporalMotion mirrors struct pt_temporal_motion_stats, and says whether the history was reset before the frame because more than
// positions and the camera had changed.
type TemporalMotion struct {
	Objects                 int // the length of the table the frame ran with; 0 = without one
	Moved, MovedReprojected uint64
	Reset                   bool
}

// SetTemporalMotion turns displaced reprojection on (pt_temporal_set_motion, DESIGN 3.13b), for an editor whose user drags objects.
// Read by Render when the accumulation is on: the frame records the object index plane (pt_set_object_ids), Render remembers the
// scene of the last frame it accumulated and compares the next one with it -- when only object positions and the camera differ, the
// displacements go to pt_temporal (nothing is passed when none is non-zero); when anything else differs the history is reset
// first.  Not set: PATHTRACER_GPU_TEMPORAL_MOTION decides.
func SetTemporalMotion(on bool) {
	mu.Lock()
	defer mu.Unlock()
	motionSet, motionOn = true, on
}

// SetFeatureWalk lets scenes on the BVH path (more than 128 spheres or 128 boxes) collect the first-hit feature planes, by a
// wave-shared walk of the tree (pt_set_feature_walk, DESIGN 3.11a): the filter's feature terms, the accumulation and the object ids
// then work there too.  Not set: PATHTRACER_GPU_FEATURE_WALK decides.
func SetFeatureWalk(on bool) {
	mu.Lock()
	defer mu.Unlock()
	walkSet, walkWanted = true, on
}

// SetFogWalk lets scenes on the BVH path (more than 128 spheres or 128 boxes) draw a gpu_volumetric fog block, the closest hit and the
// shadow rays of the term answered by wave-shared walks of the tree (pt_set_fog_walk, DESIGN 3.7a).  The frame is the model's, bit
// for bit, at 24 x lights shadow rays per sample.  Not set: PATHTRACER_GPU_FOG_WALK decides.
func SetFogWalk(on bool) {
	mu.Lock()
	defer mu.Unlock()
	fogWalkSet, fogWalkWanted = true, on
}

// SetShadingWalk lets scenes on the BVH path (more than 128 spheres or 128 boxes) render with the GL model, every closest hit,
// shadow ray and metal probe answered by the lane's own walk of the tree (pt_set_shading_walk, DESIGN 3.8a).  The frame is the
// model's, bit for bit.  Not set: PATHTRACER_GPU_SHADING_WALK decides.
func SetShadingWalk(on bool) {
	mu.Lock()
	defer mu.Unlock()
	shadingWalkSet, shadingWalkWanted = true, on
}

// SetShadingFeatures lets a GL-shaded frame take features, the a-trous filter and the filtered noise target: the features are those
// of the GL pass's own camera rays, k counts passes of 16 paths (1 under the filter unless said), and the image is GL's tone map of
// the filtered mean (pt_set_shading_features, DESIGN 3.8b).  Not set: PATHTRACER_GPU_SHADING_FEATURES decides.
func SetShadingFeatures(on bool) {
	mu.Lock()
	defer mu.Unlock()
	shadingFeaturesSet, shadingFeaturesWanted = true, on
}

// SetBvhRefit lets a frame whose scene differs from the previous frame's only in where its objects are keep the hierarchy's topology
// and recompute its boxes on the devices (pt_set_bvh_refit, DESIGN 3.4c).  maxGrowth >= 1 (or +Inf) bounds how far the refitted tree's
// quality figure may exceed the built one's before the next frame rebuilds; anything below 1 is off.  Not set:
// PATHTRACER_GPU_BVH_REFIT decides.  The library detects the refittable edits by itself.
func SetBvhRefit(maxGrowth float64) {
	mu.Lock()
	defer mu.Unlock()
	if !(maxGrowth >= 1) {
		maxGrowth = 0
	}
	refitSet, refitWanted = true, maxGrowth
}

// SetBvhBuild chooses who builds the hierarchy when a full build is due (pt_set_bvh_build, DESIGN 3.4d): the host's builder (false,
// the default) or devices[0], in Morton order (true).  The frame is the same, bit for bit.  Not set: PATHTRACER_GPU_BVH_BUILD decides.
func SetBvhBuild(device bool) {
	mu.Lock()
	defer mu.Unlock()
	buildSet, buildWanted = true, device
}

// buildRule: whether the device build is in force (SetBvhBuild, else the environment).
func buildRule() bool {
	if buildSet {
		return buildWanted
	}
	return strings.TrimSpace(os.Getenv("PATHTRACER_GPU_BVH_BUILD")) == "device"
}

// refitRule: the growth bound in force (SetBvhRefit, else the environment); 0: off.
func refitRule() float64 {
	if refitSet {
		return refitWanted
	}
	if g, err := strconv.ParseFloat(strings.TrimSpace(os.Getenv("PATHTRACER_GPU_BVH_REFIT")), 64); err == nil && g >= 1 {
		return g
	}
	return 0
}

// walkRule: whether features on the BVH path are in force (SetFeatureWalk, else the environment).
func walkRule() bool {
	if walkSet {
		return walkWanted
	}
	switch strings.ToLower(strings.TrimSpace(os.Getenv("PATHTRACER_GPU_FEATURE_WALK"))) {
	case "1", "true", "on", "yes":
		return true
	}
	return false
}

// fogWalkRule: whether volumetric fog on the BVH path is in force (SetFogWalk, else the environment).
func fogWalkRule() bool {
	if fogWalkSet {
		return fogWalkWanted
	}
	switch strings.ToLower(strings.TrimSpace(os.Getenv("PATHTRACER_GPU_FOG_WALK"))) {
	case "1", "true", "on", "yes":
		return true
	}
	return false
}

// shadingFeaturesRule: whether GL-shaded frames take features and the filter (SetShadingFeatures, else the environment).
func shadingFeaturesRule() bool {
	if shadingFeaturesSet {
		return shadingFeaturesWanted
	}
	switch strings.ToLower(strings.TrimSpace(os.Getenv("PATHTRACER_GPU_SHADING_FEATURES"))) {
	case "1", "true", "on", "yes":
		return true
	}
	return false
}

// shadingWalkRule: whether GL shading on the BVH path is in force (SetShadingWalk, else the environment).
func shadingWalkRule() bool {
	if shadingWalkSet {
		return shadingWalkWanted
	}
	switch strings.ToLower(strings.TrimSpace(os.Getenv("PATHTRACER_GPU_SHADING_WALK"))) {
	case "1", "true", "on", "yes":
		return true
	}
	return false
}

// LastTemporalMotion reports the rule's figures for the last frame Render finished (the zero value unless the rule was in force).
func LastTemporalMotion() TemporalMotion {
	mu.Lock()
	defer mu.Unlock()
	return lastMotion
}

// motionRule: whether displaced reprojection is in force (SetTemporalMotion, else the environment); only under the accumulation.
func motionRule() bool {
	if !temporalRule() {
		return false
	}
	if motionSet {
		return motionOn
	}
	switch strings.ToLower(strings.TrimSpace(os.Getenv("PATHTRACER_GPU_TEMPORAL_MOTION"))) {
	case "1", "true", "on", "yes":
		return true
	}
	return false
}

// copyScene: what sceneMotion compares, detached from the caller's scene (which the editor edits in place).
func copyScene(sc *scene.Scene) *scene.Scene {
	c := *sc
	c.Materials = append(c.Materials[:0:0], sc.Materials...)
	c.Objects = append(c.Objects[:0:0], sc.Objects...)
	if sc.Sky != nil {
		sky := *sc.Sky
		c.Sky = &sky
	}
	if sc.Fog != nil {
		fog := *sc.Fog
		c.Fog = &fog
	}
	return &c
}

// sceneMotion: delta [n][3], cur's object positions minus prev's, when the two scenes differ in object positions and the camera
// only; ok = false when anything else differs -- the number, order, type, size or material of the objects, the material table,
// sky, background or fog.
func sceneMotion(prev, cur *scene.Scene) (delta []C.double, ok bool) {
	if len(prev.Objects) != len(cur.Objects) || !reflect.DeepEqual(prev.Materials, cur.Materials) ||
		!reflect.DeepEqual(prev.Sky, cur.Sky) || !reflect.DeepEqual(prev.Fog, cur.Fog) || prev.Background != cur.Background {
		return nil, false
	}
	delta = make([]C.double, 3*len(cur.Objects))
	for i := range cur.Objects {
		a, b := prev.Objects[i], cur.Objects[i]
		if a.Type != b.Type || a.MaterialID != b.MaterialID || a.Size != b.Size {
			return nil, false
		}
		delta[3*i] = C.double(b.Position.X - a.Position.X)
		delta[3*i+1] = C.double(b.Position.Y - a.Position.Y)
		delta[3*i+2] = C.double(b.Position.Z - a.Position.Z)
	}
	return delta, true
}

// clipRule: the gamma in force (SetTemporalClip, else PATHTRACER_GPU_TEMPORAL_CLIP; unset or not a finite number >= 0: off).
func clipRule() float64 {
	if clipSet {
		return clipGamma
	}
	g, err := strconv.ParseFloat(strings.TrimSpace(os.Getenv("PATHTRACER_GPU_TEMPORAL_CLIP")), 64)
	if err != nil || math.IsNaN(g) || math.IsInf(g, 0) || g < 0 {
		return 0
	}
	return g
}

// temporalRule: whether the accumulation is in force (SetTemporal, else the environment).
func temporalRule() bool {
	if temporalSet {
		return temporalOn
	}
	switch strings.ToLower(strings.TrimSpace(os.Getenv("PATHTRACER_GPU_TEMPORAL"))) {
	case "1", "true", "on", "yes":
		return true
	}
	return false
}

// SetFeatures sets the first-hit feature samples per pixel (pt_set_features); k < 0 = not said.
func SetFeatures(k int) {
	mu.Lock()
	defer mu.Unlock()
	if k < 0 {
		k = -1
	}
	featuresK = k
}

// LastAtrous reports the filter's figures for the last frame Render finished (the zero value unless it was filtered).
func LastAtrous() AtrousStats {
	mu.Lock()
	defer mu.Unlock()
	return lastAtrous
}

// atrousRule: whether the filter is in force and its iterations (SetAtrous, else the environment).
func atrousRule() (bool, int) {
	if atrousSet {
		return atrousOn || temporalRule(), atrousIters
	}
	on, iters := temporalRule(), 5 // the accumulation brings the filter with it
	switch strings.ToLower(strings.TrimSpace(os.Getenv("PATHTRACER_GPU_ATROUS"))) {
	case "1", "true", "on", "yes":
		on = true
	}
	if v, err := strconv.Atoi(strings.TrimSpace(os.Getenv("PATHTRACER_GPU_ATROUS_ITERS"))); err == nil && v >= 0 && v <= 6 {
		iters = v
	}
	return on, iters
}

// featuresRule: the feature samples per pixel of the next frame.  Not said (SetFeatures, PATHTRACER_GPU_FEATURES): 4 under the
// filter unless the frame would refuse them (GL shading without SetShadingFeatures, a scene on the BVH path without SetFeatureWalk --
// with GL shading: without SetShadingWalk), else 0.  With GL shading k counts passes of 16 paths, and the filter's default is 1.
func featuresRule(sc *scene.Scene, atrous bool) int {
	if featuresK >= 0 {
		return featuresK
	}
	if v, err := strconv.Atoi(strings.TrimSpace(os.Getenv("PATHTRACER_GPU_FEATURES"))); err == nil && v >= 0 {
		return v
	}
	if temporalRule() {
		return 4 // pt_temporal needs them: where the frame refuses features, pt_begin says so
	}
	gl := glShading()
	if !atrous || (gl && !shadingFeaturesRule()) {
		return 0
	}
	k := 4
	if gl {
		k = 1
	}
	if (gl && shadingWalkRule()) || (!gl && walkRule()) {
		return k
	}
	spheres, boxes := 0, 0
	for _, o := range sc.Objects {
		switch o.Type {
		case scene.ObjectSphere, scene.ObjectSphereLight:
			spheres++
		case scene.ObjectBox:
			boxes++
		}
	}
	if scan := os.Getenv("PTCORE_SCAN"); spheres > 128 || boxes > 128 || scan == "bvh" || scan == "verify_bvh" {
		return 0
	}
	return k
}

// LastAdaptive reports the block table of the last frame Render finished (the zero value unless it was adaptive).
func LastAdaptive() AdaptiveState {
	mu.Lock()
	defer mu.Unlock()
	return lastAdaptive
}

// adaptiveRule: whether adaptive sampling is in force and its min_spp (SetAdaptive, else the environment).
func adaptiveRule() (bool, int) {
	if adaptiveSet {
		return adaptiveOn, adaptiveMinSpp
	}
	on, minSpp := false, 0
	switch strings.ToLower(strings.TrimSpace(os.Getenv("PATHTRACER_GPU_ADAPTIVE"))) {
	case "1", "true", "on", "yes":
		on = true
	}
	if v, err := strconv.Atoi(strings.TrimSpace(os.Getenv("PATHTRACER_GPU_ADAPTIVE_MIN_SPP"))); err == nil && v >= 0 {
		minSpp = v
	}
	return on, minSpp
}

// LastFrame reports the samples per pixel the last Render finished with and, when a noise target was set, its noise.
func LastFrame() (spp int, noise float64) {
	mu.Lock()
	defer mu.Unlock()
	return lastSpp, lastNoise
}

// noiseRule: the target and step in force (SetNoiseTarget, else the environment; 0 = off).
func noiseRule() (float64, int) {
	if noiseSet {
		return noiseTarget, noiseStep
	}
	target, step := 0.0, 16
	if v, err := strconv.ParseFloat(strings.TrimSpace(os.Getenv("PATHTRACER_GPU_NOISE")), 64); err == nil && v > 0 {
		target = v
	}
	if v, err := strconv.Atoi(strings.TrimSpace(os.Getenv("PATHTRACER_GPU_NOISE_STEP"))); err == nil && v >= 1 {
		step = v
	}
	return target, step
}

func lastError(what string) error {
	return fmt.Errorf("%s: %s", what, C.GoString(C.pt_last_error()))
}

func ensure() error {
	if ctx != nil {
		return nil
	}
	if initErr != nil {
		return initErr
	}
	if s := os.Getenv("PATHTRACER_SEED"); s != "" {
		if v, err := strconv.ParseUint(s, 10, 64); err == nil {
			seed = v
		}
	}
	if rc := C.pt_create(nil, C.int32_t(devices), &ctx); rc != C.PT_OK {
		initErr = lastError("pt_create")
		return initErr
	}
	return nil
}

func matType(t scene.MaterialType) C.int32_t {
	switch t {
	case scene.MaterialMetal:
		return C.PT_MAT_METAL
	case scene.MaterialDielectric:
		return C.PT_MAT_DIELECTRIC
	case scene.MaterialEmissive:
		return C.PT_MAT_EMISSIVE
	case scene.MaterialMirror:
		return C.PT_MAT_MIRROR
	}
	return C.PT_MAT_LAMBERT // convertMaterial's default branch, materials.go:51-53
}

func objType(t scene.ObjectType) C.int32_t {
	switch t {
	case scene.ObjectSphere:
		return C.PT_OBJ_SPHERE
	case scene.ObjectPlane:
		return C.PT_OBJ_PLANE
	case scene.ObjectBox:
		return C.PT_OBJ_BOX
	case scene.ObjectSphereLight:
		return C.PT_OBJ_SPHERE_LIGHT
	}
	return C.PT_OBJ_UNKNOWN // skipped by sceneToWorld, objects.go:237-266
}

func set3(d *[3]C.double, x, y, z float64) { d[0], d[1], d[2] = C.double(x), C.double(y), C.double(z) }

// flatten copies the scene into C memory (freed by the returned func): C never sees a Go pointer
// to memory containing Go pointers.
func flatten(sc *scene.Scene) (*C.pt_scene, func()) {
	nm, no := len(sc.Materials), len(sc.Objects)
	cs := (*C.pt_scene)(C.calloc(1, C.size_t(unsafe.Sizeof(C.pt_scene{}))))
	var mats *C.pt_material
	var objs *C.pt_object
	ids := make(map[string]int, nm)
	if nm > 0 {
		mats = (*C.pt_material)(C.calloc(C.size_t(nm), C.size_t(unsafe.Sizeof(C.pt_material{}))))
		ms := unsafe.Slice(mats, nm)
		for i, m := range sc.Materials {
			ms[i]._type = matType(m.Type)
			set3(&ms[i].albedo, m.Albedo.R, m.Albedo.G, m.Albedo.B)
			ms[i].rough = C.double(m.Rough)
			ms[i].ior = C.double(m.IOR)
			set3(&ms[i].emit, m.Emit.R, m.Emit.G, m.Emit.B)
			ms[i].power = C.double(m.Power)
			set3(&ms[i].absorption, m.Absorption.R, m.Absorption.G, m.Absorption.B)
			ms[i].smoothness = C.double(m.Smoothness)
			ids[m.ID] = i // the last duplicate wins, like the map at objects.go:227-229
		}
	}
	if no > 0 {
		objs = (*C.pt_object)(C.calloc(C.size_t(no), C.size_t(unsafe.Sizeof(C.pt_object{}))))
		os_ := unsafe.Slice(objs, no)
		for i, o := range sc.Objects {
			os_[i]._type = objType(o.Type)
			if k, ok := ids[o.MaterialID]; ok {
				os_[i].material = C.int32_t(k)
			} else {
				os_[i].material = -1
			}
			set3(&os_[i].position, o.Position.X, o.Position.Y, o.Position.Z)
			set3(&os_[i].size, o.Size.X, o.Size.Y, o.Size.Z)
		}
	}
	c := sc.Camera
	set3(&cs.camera.position, c.Position.X, c.Position.Y, c.Position.Z)
	set3(&cs.camera.target, c.Target.X, c.Target.Y, c.Target.Z)
	set3(&cs.camera.up, c.Up.X, c.Up.Y, c.Up.Z)
	cs.camera.fov = C.double(c.FOV)
	cs.camera.aperture = C.double(c.Aperture)
	cs.camera.focus_dist = C.double(c.FocusDist)
	cs.camera.aspect_ratio = C.double(c.AspectRatio)
	set3(&cs.sky.background, sc.Background.R, sc.Background.G, sc.Background.B)
	cs.sky.kind = C.PT_SKY_BACKGROUND
	if sc.Sky != nil {
		switch sc.Sky.Type {
		case "gradient":
			cs.sky.kind = C.PT_SKY_GRADIENT
		case "solid":
			cs.sky.kind = C.PT_SKY_SOLID
		}
		set3(&cs.sky.color, sc.Sky.Color.R, sc.Sky.Color.G, sc.Sky.Color.B)
		set3(&cs.sky.horizon, sc.Sky.Horizon.R, sc.Sky.Horizon.G, sc.Sky.Horizon.B)
		set3(&cs.sky.zenith, sc.Sky.Zenith.R, sc.Sky.Zenith.G, sc.Sky.Zenith.B)
	}
	cs.num_materials = C.int32_t(nm)
	cs.num_objects = C.int32_t(no)
	cs.materials = mats
	cs.objects = objs
	return cs, func() {
		C.free(unsafe.Pointer(mats))
		C.free(unsafe.Pointer(objs))
		C.free(unsafe.Pointer(cs))
	}
}

// fogEnabled: PATHTRACER_GPU_FOG=1 (true / on / yes) draws the scene's fog block the way the GL backend does
// (gpu.go:1125-1341); without it fog is ignored, like the CPU engine ignores it (scene.go:100).
func fogEnabled() bool {
	switch os.Getenv("PATHTRACER_GPU_FOG") {
	case "1", "true", "TRUE", "True", "on", "ON", "yes", "YES":
		return true
	}
	return false
}

// setFog hands sc.Fog to the context (pt_set_fog), or turns fog off.  pt_fog holds no pointers.
func setFog(sc *scene.Scene) error {
	if !fogEnabled() || sc.Fog == nil {
		if rc := C.pt_set_fog(ctx, nil); rc != C.PT_OK {
			return lastError("pt_set_fog")
		}
		return nil
	}
	f := sc.Fog
	var cf C.pt_fog
	cf.density = C.double(f.Density)
	set3(&cf.color, f.Color.R, f.Color.G, f.Color.B)
	cf.scatter = C.double(f.Scatter)
	cf.sigma_s = C.double(f.SigmaS)
	cf.sigma_a = C.double(f.SigmaA)
	cf.g = C.double(f.G)
	cf.hetero_strength = C.double(f.HeteroStrength)
	cf.noise_scale = C.double(f.NoiseScale)
	cf.noise_octaves = C.int32_t(f.NoiseOctaves)
	if f.AffectSky {
		cf.affect_sky = 1
	}
	if f.GPUVolumetric {
		cf.gpu_volumetric = 1
	}
	if rc := C.pt_set_fog(ctx, &cf); rc != C.PT_OK {
		return lastError("pt_set_fog")
	}
	return nil
}

// glShading: PATHTRACER_GPU_SHADING=gl (any case) renders with the GL backend's estimator (gpu.go:1300-1732) instead of
// the CPU engine's; a "sample" is then a pass of 16 paths and the image is the GL finish (DESIGN 3.8).
func glShading() bool {
	return strings.EqualFold(strings.TrimSpace(os.Getenv("PATHTRACER_GPU_SHADING")), "gl")
}

// setShading selects the context's shading model (pt_set_shading).  For GL shading it hands over the per-material fields
// only that model reads; the table is copied by the call.
func setShading(sc *scene.Scene) error {
	if !glShading() {
		if rc := C.pt_set_shading(ctx, nil); rc != C.PT_OK {
			return lastError("pt_set_shading")
		}
		return nil
	}
	n := len(sc.Materials)
	var tab *C.pt_gl_material
	if n > 0 {
		tab = (*C.pt_gl_material)(C.malloc(C.size_t(n) * C.size_t(unsafe.Sizeof(C.pt_gl_material{}))))
		defer C.free(unsafe.Pointer(tab))
		gm := unsafe.Slice(tab, n)
		for i, m := range sc.Materials {
			gm[i].reflectivity = C.double(m.Reflectivity)
			set3(&gm[i].tint, m.Tint.R, m.Tint.G, m.Tint.B)
			gm[i].absorption_scale = C.double(m.AbsorptionScale)
		}
	}
	s := C.pt_shading{model: C.PT_SHADING_GL, num_materials: C.int32_t(n), materials: tab}
	if rc := C.pt_set_shading(ctx, &s); rc != C.PT_OK {
		return lastError("pt_set_shading")
	}
	return nil
}

// Render renders sc into img on the MI355X and calls progress() every ~10% of the samples and once
// at the end (the cadence of gpu.go:2209-2212, :2229, :2523-2525).  On any error the caller
// (engine.renderIntoGPU) falls back to the CPU renderer exactly as it does for the GL backend.
func Render(sc *scene.Scene, cfg RenderConfig, img *image.RGBA, progress func()) error {
	err := renderFrame(sc, cfg, img, progress)
	if err != nil || sc == nil || img == nil || len(img.Pix) == 0 {
		return err
	}
	mu.Lock()
	defer mu.Unlock()
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	lastAtrous = AtrousStats{}
	lastTemporal = TemporalStats{}
	lastMotion = TemporalMotion{}
	if _, iters := atrousRule(); temporalRule() && ctx != nil && img.Bounds().Dx() == cfg.Width && img.Bounds().Dy() == cfg.Height {
		// the frame blended into the context's reprojected history, then filtered, takes the place of the plain finish
		ac := C.pt_atrous_config{iterations: C.int32_t(iters), sigma_l: 4, sigma_n: 0.1, sigma_z: 0.1, sigma_a: 0.2}
		var tc *C.pt_temporal_config // nil: the defaults
		var st C.pt_temporal_stats
		if rc := C.pt_temporal_set_clip(ctx, C.double(clipRule())); rc != C.PT_OK {
			return lastError("pt_temporal_set_clip")
		}
		motion, table := motionRule(), false
		if motion && accumulated != nil { // the host rule of displaced reprojection (DESIGN 3.13b)
			delta, ok := sceneMotion(accumulated, sc)
			moved := false
			for _, d := range delta {
				moved = moved || d != 0
			}
			if !ok {
				lastMotion.Reset = true
				if rc := C.pt_temporal_reset(ctx); rc != C.PT_OK {
					return lastError("pt_temporal_reset")
				}
			} else if moved { // (a Go slice of C.double holds no Go pointers: it may be passed directly)
				if rc := C.pt_temporal_set_motion(ctx, &delta[0], C.int32_t(len(delta)/3)); rc != C.PT_OK {
					return lastError("pt_temporal_set_motion")
				}
				table = true
			}
		}
		if rc := C.pt_temporal(ctx, tc, &ac, (*C.uint8_t)(unsafe.Pointer(&img.Pix[0])), C.int32_t(img.Stride), nil, nil, &st); rc != C.PT_OK {
			return lastError("pt_temporal")
		}
		lastTemporal = TemporalStats{Ms: float64(st.temporal_ms), Launches: int(st.launches), Iterations: int(st.iterations),
			Reprojected: uint64(st.reprojected), Disoccluded: uint64(st.disoccluded), BadPixels: uint64(st.bad_pixels),
			MeanLen: float64(st.mean_len), NoiseBefore: float64(st.noise_before), NoiseBlended: float64(st.noise_blended),
			NoiseAfter: float64(st.noise_after)}
		accumulated = nil // (a frame accumulated without the rule is not what the next table is against)
		if table {
			var ms C.struct_pt_temporal_motion_stats
			if rc := C.pt_temporal_motion_stats(ctx, &ms); rc != C.PT_OK {
				return lastError("pt_temporal_motion_stats")
			}
			lastMotion.Objects, lastMotion.Moved, lastMotion.MovedReprojected = int(ms.objects), uint64(ms.moved), uint64(ms.moved_reprojected)
		}
		if motion {
			accumulated = copyScene(sc)
		}
		if progress != nil {
			progress()
		}
		return nil
	}
	if on, iters := atrousRule(); on && ctx != nil && img.Bounds().Dx() == cfg.Width && img.Bounds().Dy() == cfg.Height {
		// the filtered image takes the place of the plain finish (the sums stay readable after pt_end)
		ac := C.pt_atrous_config{iterations: C.int32_t(iters), sigma_l: 4, sigma_n: 0.1, sigma_z: 0.1, sigma_a: 0.2}
		var st C.pt_atrous_stats
		if rc := C.pt_atrous(ctx, &ac, (*C.uint8_t)(unsafe.Pointer(&img.Pix[0])), C.int32_t(img.Stride), nil, nil, &st); rc != C.PT_OK {
			return lastError("pt_atrous")
		}
		lastAtrous = AtrousStats{Ms: float64(st.atrous_ms), Launches: int(st.launches), Iterations: int(st.iterations),
			NoiseBefore: float64(st.noise_before), NoiseAfter: float64(st.noise_after), BadPixels: uint64(st.bad_pixels),
			Features: featuresRule(sc, true)}
		if progress != nil {
			progress()
		}
	}
	return nil
}

// renderFrame: the frame itself (Render adds the a-trous filter behind it when that is on).
func renderFrame(sc *scene.Scene, cfg RenderConfig, img *image.RGBA, progress func()) error {
	if sc == nil || img == nil {
		return errors.New("hip.Render: nil scene or image")
	}
	b := img.Bounds()
	if b.Dx() != cfg.Width || b.Dy() != cfg.Height {
		return nil // renderIntoCPU silently returns on a size mismatch (renderer.go:46-49)
	}
	if len(img.Pix) == 0 {
		return errors.New("hip.Render: empty image")
	}
	mu.Lock()
	defer mu.Unlock()
	// pt_last_error() is thread-local on the C side: stay on one OS thread from a failing call to its message
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if err := ensure(); err != nil {
		return err
	}
	cs, free := flatten(sc)
	defer free()
	if err := setFog(sc); err != nil {
		return err
	}
	if err := setShading(sc); err != nil {
		return err
	}
	target, nstep := noiseRule()
	toNoise := target > 0
	atrous, atrousN := atrousRule()
	filtered := filteredRule()
	blockTarget, pool := filteredAdaptiveRule()
	if blockTarget > 0 && (toNoise || filtered > 0) {
		return errors.New("hip.Render: the filtered adaptive target excludes a frame noise target, adaptive sampling and the filtered noise target: one stop rule per frame")
	}
	if blockTarget > 0 && glShading() {
		return errors.New("hip.Render: the filtered adaptive target is not available with GL shading")
	}
	if filtered > 0 && toNoise {
		return errors.New("hip.Render: the filtered noise target excludes a frame noise target and adaptive sampling: one stop rule per frame")
	}
	if filtered > 0 && glShading() && !shadingFeaturesRule() {
		return errors.New("hip.Render: the filtered noise target is not available with GL shading")
	}
	var halvesOn C.int32_t
	if filtered > 0 {
		halvesOn = 1
	}
	if rc := C.pt_set_halves(ctx, halvesOn); rc != C.PT_OK {
		return lastError("pt_set_halves")
	}
	if walk := walkRule(); walk != walkOn { // (said only when the switch changes: with it never on, the calls are what they were)
		var w C.int32_t
		if walk {
			w = 1
		}
		if rc := C.pt_set_feature_walk(ctx, w); rc != C.PT_OK {
			return lastError("pt_set_feature_walk")
		}
		walkOn = walk
	}
	if walk := fogWalkRule(); walk != fogWalkOn { // (the same: said only when the switch changes)
		var w C.int32_t
		if walk {
			w = 1
		}
		if rc := C.pt_set_fog_walk(ctx, w); rc != C.PT_OK {
			return lastError("pt_set_fog_walk")
		}
		fogWalkOn = walk
	}
	if walk := shadingWalkRule(); walk != shadingWalkOn { // (the same)
		var w C.int32_t
		if walk {
			w = 1
		}
		if rc := C.pt_set_shading_walk(ctx, w); rc != C.PT_OK {
			return lastError("pt_set_shading_walk")
		}
		shadingWalkOn = walk
	}
	if feat := shadingFeaturesRule(); feat != shadingFeaturesOn { // (the same)
		var w C.int32_t
		if feat {
			w = 1
		}
		if rc := C.pt_set_shading_features(ctx, w); rc != C.PT_OK {
			return lastError("pt_set_shading_features")
		}
		shadingFeaturesOn = feat
	}
	if g := refitRule(); g != refitSaid { // (the same: said only when the bound changes)
		if rc := C.pt_set_bvh_refit(ctx, C.double(g)); rc != C.PT_OK {
			return lastError("pt_set_bvh_refit")
		}
		refitSaid = g
	}
	if b := buildRule(); b != buildSaid { // (the same: said only when the mode changes)
		mode := C.int32_t(0)
		if b {
			mode = 1
		}
		if rc := C.pt_set_bvh_build(ctx, mode); rc != C.PT_OK {
			return lastError("pt_set_bvh_build")
		}
		buildSaid = b
	}
	if rc := C.pt_set_features(ctx, C.int32_t(featuresRule(sc, atrous))); rc != C.PT_OK {
		return lastError("pt_set_features")
	}
	if motion := motionRule(); motion != idsOn { // (said only when the switch changes: with it never on, the calls are what they were)
		var ids C.int32_t
		if motion {
			ids = 1
		}
		if rc := C.pt_set_object_ids(ctx, ids); rc != C.PT_OK {
			return lastError("pt_set_object_ids")
		}
		idsOn = motion
	}
	var on C.int32_t
	if toNoise || atrous { // the filter reads the second moments
		on = 1
	}
	if rc := C.pt_set_moments(ctx, on); rc != C.PT_OK {
		return lastError("pt_set_moments")
	}
	adaptive, minSpp := adaptiveRule()
	adaptive = adaptive && toNoise // the noise target is the blocks' target
	if blockTarget > 0 { // an adaptive frame whose blocks stop by the filtered frame's pooled noise
		adaptive, toNoise, target = true, true, blockTarget
	}
	if blockTarget > 0 || filteredAdaptiveOn {
		if blockTarget > 0 {
			fa := C.pt_adaptive_filtered{filter: C.pt_atrous_config{iterations: C.int32_t(atrousN), sigma_l: 4, sigma_n: 0.1, sigma_z: 0.1, sigma_a: 0.2},
				pool: C.int32_t(pool)}
			if rc := C.pt_set_adaptive_filtered(ctx, &fa); rc != C.PT_OK {
				return lastError("pt_set_adaptive_filtered")
			}
		} else if rc := C.pt_set_adaptive_filtered(ctx, nil); rc != C.PT_OK {
			return lastError("pt_set_adaptive_filtered")
		}
		filteredAdaptiveOn = blockTarget > 0
	}
	if adaptive {
		ad := C.pt_adaptive{target: C.double(target), min_spp: C.int32_t(minSpp), step: C.int32_t(nstep)}
		if rc := C.pt_set_adaptive(ctx, &ad); rc != C.PT_OK {
			return lastError("pt_set_adaptive")
		}
	} else if rc := C.pt_set_adaptive(ctx, nil); rc != C.PT_OK {
		return lastError("pt_set_adaptive")
	}
	lastSpp, lastNoise, lastAdaptive, lastHalves = 0, 0, AdaptiveState{}, HalvesStats{}
	pc := C.pt_config{width: C.int32_t(cfg.Width), height: C.int32_t(cfg.Height),
		samples_per_px: C.int32_t(cfg.SamplesPerPx), max_depth: C.int32_t(cfg.MaxDepth), seed: C.uint64_t(seed)}
	pix := (*C.uint8_t)(unsafe.Pointer(&img.Pix[0]))
	if toNoise {
		return renderToNoise(cs, &pc, cfg, img, pix, progress, target, nstep, adaptive, blockTarget <= 0)
	}
	if filtered > 0 {
		return renderToFilteredNoise(cs, &pc, cfg, img, pix, progress, filtered, nstep, atrousN)
	}
	if progress == nil {
		if rc := C.pt_render(ctx, cs, &pc, pix, C.int32_t(img.Stride), nil, nil, nil, nil); rc != C.PT_OK {
			return lastError("pt_render")
		}
		lastSpp = cfg.SamplesPerPx
		return nil
	}
	if rc := C.pt_begin(ctx, cs, &pc); rc != C.PT_OK {
		return lastError("pt_begin")
	}
	step := cfg.SamplesPerPx / 10
	if step < 1 {
		step = 1
	}
	var done C.int32_t
	var err error
	for int(done) < cfg.SamplesPerPx {
		if rc := C.pt_step(ctx, C.int32_t(step), &done); rc != C.PT_OK {
			err = lastError("pt_step")
			break
		}
		if rc := C.pt_read(ctx, pix, C.int32_t(img.Stride), nil); rc != C.PT_OK {
			err = lastError("pt_read")
			break
		}
		progress()
	}
	if err == nil && cfg.SamplesPerPx <= 0 {
		// zero samples: the reference's pixel finish of an empty sum (renderer.go:190-221)
		if rc := C.pt_read(ctx, pix, C.int32_t(img.Stride), nil); rc != C.PT_OK {
			err = lastError("pt_read")
		}
	}
	if rc := C.pt_end(ctx, nil); rc != C.PT_OK && err == nil {
		err = lastError("pt_end")
	}
	if err == nil {
		progress()
		lastSpp = int(done)
	}
	return err
}

// renderToFilteredNoise: pt_begin with cfg.SamplesPerPx as the cap, then steps of nstep samples; after each step with at least 4
// samples done pt_atrous_halves measures the noise of the filtered frame, and the loop stops at the first check at or below target.
// Called with mu held on a locked OS thread.
func renderToFilteredNoise(cs *C.pt_scene, pc *C.pt_config, cfg RenderConfig, img *image.RGBA, pix *C.uint8_t, progress func(),
	target float64, nstep int, iters int) error {
	if rc := C.pt_begin(ctx, cs, pc); rc != C.PT_OK {
		return lastError("pt_begin")
	}
	ac := C.pt_atrous_config{iterations: C.int32_t(iters), sigma_l: 4, sigma_n: 0.1, sigma_z: 0.1, sigma_a: 0.2}
	var done C.int32_t
	var hs C.pt_halves_stats
	var err error
	for int(done) < cfg.SamplesPerPx {
		n := cfg.SamplesPerPx - int(done)
		if nstep < n {
			n = nstep
		}
		if rc := C.pt_step(ctx, C.int32_t(n), &done); rc != C.PT_OK {
			err = lastError("pt_step")
			break
		}
		if progress != nil {
			if rc := C.pt_read(ctx, pix, C.int32_t(img.Stride), nil); rc != C.PT_OK {
				err = lastError("pt_read")
				break
			}
			progress()
		}
		if int(done) < 4 { // each half needs two samples for its variance
			continue
		}
		if rc := C.pt_atrous_halves(ctx, &ac, nil, nil, nil, &hs); rc != C.PT_OK {
			err = lastError("pt_atrous_halves")
			break
		}
		if float64(hs.noise) <= target {
			break
		}
	}
	if err == nil && (progress == nil || cfg.SamplesPerPx <= 0) {
		if rc := C.pt_read(ctx, pix, C.int32_t(img.Stride), nil); rc != C.PT_OK {
			err = lastError("pt_read")
		}
	}
	if rc := C.pt_end(ctx, nil); rc != C.PT_OK && err == nil {
		err = lastError("pt_end")
	}
	if err == nil {
		if progress != nil {
			progress()
		}
		lastSpp = int(done)
		lastHalves = HalvesStats{Ms: float64(hs.atrous_ms), Launches: int(hs.launches), Iterations: int(hs.iterations), Noise: float64(hs.noise),
			NoiseModel: float64(hs.noise_model), BadPixels: uint64(hs.bad_pixels), SppMin: int(hs.spp_min)}
	}
	return err
}

// renderToNoise: pt_begin with cfg.SamplesPerPx as the cap, then steps of nstep samples with a noise check after each;
// stops at the first check with at least 2 samples done and noise <= target.  The image is that of a frame of the
// samples done.  With adaptive the blocks stop inside pt_step and the loop ends when a step adds nothing.  Called with mu held
// on a locked OS thread.
func renderToNoise(cs *C.pt_scene, pc *C.pt_config, cfg RenderConfig, img *image.RGBA, pix *C.uint8_t, progress func(),
	target float64, nstep int, adaptive bool, measure bool) error {
	if rc := C.pt_begin(ctx, cs, pc); rc != C.PT_OK {
		return lastError("pt_begin")
	}
	var done C.int32_t
	var nz C.pt_noise
	var err error
	for int(done) < cfg.SamplesPerPx {
		n := cfg.SamplesPerPx - int(done)
		if nstep < n {
			n = nstep
		}
		before := done
		if rc := C.pt_step(ctx, C.int32_t(n), &done); rc != C.PT_OK {
			err = lastError("pt_step")
			break
		}
		if adaptive && done == before { // every block has stopped
			break
		}
		if progress != nil {
			if rc := C.pt_read(ctx, pix, C.int32_t(img.Stride), nil); rc != C.PT_OK {
				err = lastError("pt_read")
				break
			}
			progress()
		}
		if !measure { // the blocks stop inside pt_step by the filtered frame's pooled noise: the frame noise decides nothing
			continue
		}
		if rc := C.pt_noise_estimate(ctx, &nz); rc != C.PT_OK {
			err = lastError("pt_noise_estimate")
			break
		}
		if !adaptive && int(done) >= 2 && float64(nz.noise) <= target {
			break
		}
	}
	var as C.struct_pt_adaptive_state
	if adaptive && err == nil {
		if rc := C.pt_adaptive_state(ctx, &as); rc != C.PT_OK {
			err = lastError("pt_adaptive_state")
		}
	}
	if err == nil && (progress == nil || cfg.SamplesPerPx <= 0) {
		if rc := C.pt_read(ctx, pix, C.int32_t(img.Stride), nil); rc != C.PT_OK {
			err = lastError("pt_read")
		}
	}
	if rc := C.pt_end(ctx, nil); rc != C.PT_OK && err == nil {
		err = lastError("pt_end")
	}
	if err == nil {
		if progress != nil {
			progress()
		}
		lastSpp, lastNoise = int(done), float64(nz.noise)
		if adaptive {
			lastAdaptive = AdaptiveState{Blocks: uint64(as.blocks), ActiveBlocks: uint64(as.active_blocks), Samples: uint64(as.samples),
				SppMin: int(as.spp_min), SppMax: int(as.spp_max), WorstActive: float64(as.worst_active)}
		}
	}
	return err
}
