// Headless twin of the reference's cmd/render (cmd/render/main.go:14-63) with the UI behind a build
// tag, so the binary needs only libc and libptcore.so.  NOT COMPILED IN THE BUILD IMAGE (no Go).
//
// Reference flags kept verbatim: -scene -mode -gpu -headless -out.
// Additive flags: -width -height -spp -depth (override the mode preset), -seed, -devices,
// -scene-settings (the editor's scene-settings override, internal/ui/app.go:60-75; off = main.go:52),
// -noise -noise-step (render until the frame noise is at or below the target, -spp being the cap; DESIGN 3.9),
// -adaptive -min-spp (with -noise: every 8x8 block stops at the target by itself; DESIGN 3.10).
// -atrous -atrous-iters -features (the variance-guided a-trous filtered image and its first-hit feature samples; DESIGN 3.11).
// -filtered-noise (with -atrous: render until the measured noise of the filtered frame is at or below the target; DESIGN 3.12).
// -feature-walk (features on scenes that take the BVH path, by a wave-shared walk of the tree; DESIGN 3.11a).
package main

import (
	"flag"
	"fmt"
	"log"
	"os"

	"github.com/user/pathtracer/internal/engine"
	"github.com/user/pathtracer/internal/engine/hip"
	"github.com/user/pathtracer/internal/scene"
)

func main() {
	log.Println("pathtracer: starting main()")
	scenePath := flag.String("scene", "scenes/example_simple.json", "path to scene JSON file")
	mode := flag.String("mode", "preview", "render mode: preview or final")
	useGPU := flag.Bool("gpu", false, "use GPU backend for rendering (if available)")
	headless := flag.Bool("headless", false, "render without UI and save PNG")
	output := flag.String("out", "output.png", "output PNG file for headless render")
	width := flag.Int("width", 0, "image width (default: the mode preset)")
	height := flag.Int("height", 0, "image height (default: the mode preset)")
	spp := flag.Int("spp", -1, "samples per pixel (default: the mode preset)")
	depth := flag.Int("depth", -1, "max path depth (default: the mode preset)")
	seed := flag.Uint64("seed", 1, "sample-stream seed")
	devices := flag.Int("devices", 1, "number of GPUs to tile the image over")
	sceneSettings := flag.Bool("scene-settings", false, "let the scene file's settings block override the mode preset")
	noise := flag.Float64("noise", 0, "render until the frame noise is at or below this target, -spp being the cap (0 = off, or PATHTRACER_GPU_NOISE)")
	noiseStep := flag.Int("noise-step", 16, "samples per pixel between two noise checks (or PATHTRACER_GPU_NOISE_STEP)")
	adaptive := flag.Bool("adaptive", false, "with -noise: stop every 8x8 block at the target by itself (or PATHTRACER_GPU_ADAPTIVE)")
	minSpp := flag.Int("min-spp", 0, "with -adaptive: samples every block gets before the first check (or PATHTRACER_GPU_ADAPTIVE_MIN_SPP)")
	atrous := flag.Bool("atrous", false, "write the variance-guided a-trous filtered image (or PATHTRACER_GPU_ATROUS)")
	atrousIters := flag.Int("atrous-iters", 5, "with -atrous: iterations 0..6 (or PATHTRACER_GPU_ATROUS_ITERS)")
	features := flag.Int("features", -1, "first-hit feature samples per pixel (default: 4 with -atrous where the scene allows them, else 0; or PATHTRACER_GPU_FEATURES)")
	filteredNoise := flag.Float64("filtered-noise", 0, "with -atrous: render until the measured noise of the filtered frame is at or below this target, checking every -noise-step samples, -spp being the cap (0 = off, or PATHTRACER_GPU_FILTERED_NOISE)")
	bvhRefit := flag.Float64("bvh-refit", 0, "refit the bounding-volume hierarchy on the GPU when a scene's objects only moved; the value (>= 1, or +Inf) bounds how far the tree may degrade before it is rebuilt (or PATHTRACER_GPU_BVH_REFIT)")
	bvhBuild := flag.String("bvh-build", "host", "who builds the bounding-volume hierarchy when a full build is due: host, or device (the GPU, in Morton order; or PATHTRACER_GPU_BVH_BUILD)")
	featureWalk := flag.Bool("feature-walk", false, "collect features on scenes beyond 128 spheres or 128 boxes too, by a wave-shared walk of the tree (or PATHTRACER_GPU_FEATURE_WALK)")
	fogWalk := flag.Bool("fog-walk", false, "with -fog: draw a gpu_volumetric fog block on scenes beyond 128 spheres or 128 boxes too, the shadow rays by a wave-shared walk of the tree (or PATHTRACER_GPU_FOG_WALK)")
	shadingWalk := flag.Bool("shading-walk", false, "with -shading gl: render scenes beyond 128 spheres or 128 boxes too, the model's ray queries by the lane's own walk of the tree (or PATHTRACER_GPU_SHADING_WALK)")
	shadingFeatures := flag.Bool("shading-features", false, "with -shading gl: let the frame take -features and -atrous, the features being those of the GL pass's own camera rays (or PATHTRACER_GPU_SHADING_FEATURES)")
	flag.Parse()
	log.Printf("flags: scene=%s mode=%s headless=%v out=%s\n", *scenePath, *mode, *headless, *output)

	if *useGPU {
		engine.SetBackend(engine.BackendGPU) // RenderInto -> renderIntoGPU -> hip.Render (see INTEGRATION.md)
		hip.SetDevices(*devices)
		hip.SetSeed(*seed)
		noiseGiven := false
		flag.Visit(func(f *flag.Flag) { noiseGiven = noiseGiven || f.Name == "noise" || f.Name == "noise-step" })
		if noiseGiven { // else the environment decides
			hip.SetNoiseTarget(*noise, *noiseStep)
		}
		adaptiveGiven := false
		flag.Visit(func(f *flag.Flag) { adaptiveGiven = adaptiveGiven || f.Name == "adaptive" || f.Name == "min-spp" })
		if adaptiveGiven { // else the environment decides
			hip.SetAdaptive(*adaptive, *minSpp)
		}
		atrousGiven, featuresGiven := false, false
		flag.Visit(func(f *flag.Flag) {
			atrousGiven = atrousGiven || f.Name == "atrous" || f.Name == "atrous-iters"
			featuresGiven = featuresGiven || f.Name == "features"
		})
		if atrousGiven { // else the environment decides
			hip.SetAtrous(*atrous, *atrousIters)
		}
		if featuresGiven {
			hip.SetFeatures(*features)
		}
		walkGiven := false
		flag.Visit(func(f *flag.Flag) { walkGiven = walkGiven || f.Name == "feature-walk" })
		if walkGiven { // else the environment decides
			hip.SetFeatureWalk(*featureWalk)
		}
		fogWalkGiven := false
		flag.Visit(func(f *flag.Flag) { fogWalkGiven = fogWalkGiven || f.Name == "fog-walk" })
		if fogWalkGiven { // else the environment decides
			hip.SetFogWalk(*fogWalk)
		}
		shadingWalkGiven := false
		flag.Visit(func(f *flag.Flag) { shadingWalkGiven = shadingWalkGiven || f.Name == "shading-walk" })
		if shadingWalkGiven { // else the environment decides
			hip.SetShadingWalk(*shadingWalk)
		}
		shadingFeaturesGiven := false
		flag.Visit(func(f *flag.Flag) { shadingFeaturesGiven = shadingFeaturesGiven || f.Name == "shading-features" })
		if shadingFeaturesGiven { // else the environment decides
			hip.SetShadingFeatures(*shadingFeatures)
		}
		refitGiven := false
		flag.Visit(func(f *flag.Flag) { refitGiven = refitGiven || f.Name == "bvh-refit" })
		if refitGiven { // else the environment decides
			hip.SetBvhRefit(*bvhRefit)
		}
		buildGiven := false
		flag.Visit(func(f *flag.Flag) { buildGiven = buildGiven || f.Name == "bvh-build" })
		if buildGiven { // else the environment decides
			if *bvhBuild != "host" && *bvhBuild != "device" {
				log.Fatalf("invalid value %q for flag -bvh-build: want host or device", *bvhBuild)
			}
			hip.SetBvhBuild(*bvhBuild == "device")
		}
		filteredGiven := false
		flag.Visit(func(f *flag.Flag) { filteredGiven = filteredGiven || f.Name == "filtered-noise" })
		if filteredGiven { // else the environment decides
			hip.SetFilteredNoise(*filteredNoise)
		}
	} else {
		engine.SetBackend(engine.BackendCPU)
	}
	if !*headless {
		log.Println("ui error: built without the ui tag; use -headless")
		os.Exit(1)
	}
	sc, err := scene.Load(*scenePath)
	if err != nil {
		log.Println("headless render error:", fmt.Errorf("load scene: %w", err))
		os.Exit(1)
	}
	s := engine.RenderSettingsForMode(*mode)
	if *sceneSettings { // internal/ui/app.go:60-75
		if sc.Settings.Width > 0 && sc.Settings.Height > 0 {
			s.Width, s.Height = sc.Settings.Width, sc.Settings.Height
			if sc.Settings.SamplesPerPx > 0 {
				s.SamplesPerPx = sc.Settings.SamplesPerPx
			}
			if sc.Settings.MaxDepth > 0 {
				s.MaxDepth = sc.Settings.MaxDepth
			}
		}
		if *mode == "final" {
			s.SamplesPerPx *= 4
			s.MaxDepth *= 2
		}
	}
	if *width > 0 {
		s.Width = *width
	}
	if *height > 0 {
		s.Height = *height
	}
	if *spp >= 0 {
		s.SamplesPerPx = *spp
	}
	if *depth >= 0 {
		s.MaxDepth = *depth
	}
	img, err := engine.RenderScene(sc, s)
	if err != nil {
		log.Println("headless render error:", fmt.Errorf("render scene: %w", err))
		os.Exit(1)
	}
	if *useGPU {
		if a := hip.LastAdaptive(); a.Blocks > 0 {
			n, z := hip.LastFrame()
			log.Printf("rendered %dx%d, %d to %d of at most %d spp per 8x8 block (adaptive: %d of %d blocks still above the target; frame noise %.6g)\n",
				s.Width, s.Height, a.SppMin, n, s.SamplesPerPx, a.ActiveBlocks, a.Blocks, z)
		} else if h := hip.LastHalves(); h.Launches > 0 {
			n, _ := hip.LastFrame()
			log.Printf("rendered %dx%d, %d of at most %d spp (filtered noise %.6g measured, %.6g propagated)\n", s.Width, s.Height, n, s.SamplesPerPx,
				h.Noise, h.NoiseModel)
		} else if n, z := hip.LastFrame(); z > 0 {
			log.Printf("rendered %dx%d, %d of at most %d spp (noise %.6g)\n", s.Width, s.Height, n, s.SamplesPerPx, z)
		}
	}
	if err := engine.SavePNG(*output, img); err != nil {
		log.Println("headless render error:", fmt.Errorf("save png: %w", err))
		os.Exit(1)
	}
}
