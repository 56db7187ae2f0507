-- A moving WORLD in the vocabulary of orbit_animation.lua: the camera stands still while two balls bounce over a checked
-- floor and the light swings above them, one encoder:AddFrame(world, camera) per step. Every frame is another world, so
-- every job but the first reports same_world_as_previous == false — the sequence rtc_world_update is for.
-- Written for this repository (tests/test_host_world_update.py, tests/test_gpu_world_update.py).
FRAMES = FRAMES or 24          -- a caller may preset these globals by prepending assignments
BALLS = BALLS or 0             -- bystanders that stay where they are
ONLY_RED = ONLY_RED or false   -- true: the red ball alone moves (one moving sphere among the bystanders)
WIDTH, HEIGHT = WIDTH or 320, HEIGHT or 200

local MATT = { ambient = 0.1, diffuse = 0.8, specular = 0.2, shininess = 40.0 }
local MIRROR = { ambient = 0.05, diffuse = 0.4, specular = 0.9, shininess = 250.0, reflectiveness = 0.4 }

-- The closed forms of the motion, t = frame / FRAMES in [0, 1): a ball of radius r touches the floor `hops` times.
function ball_height(t, r, top, hops) return r + top * math.abs(math.sin(math.pi * hops * t)) end
function light_x(t) return -6 + 5 * math.sin(2 * math.pi * t) end

local red = { type = "sphere", material = MATT, color = { r = 0.9, g = 0.2, b = 0.2 }, scale = 0.7, position = { x = -1.2, y = 0.7, z = 0 } }
local steel = { type = "sphere", material = MIRROR, color = { r = 0.6, g = 0.65, b = 0.7 }, scale = 0.5, position = { x = 1.1, y = 0.5, z = -0.6 } }

world = {
   lights = { { color = { r = 1, g = 1, b = 1 }, position = { x = -6, y = 9, z = -7 } } },
   shapes = {
      { type = "plane", material = { specular = 0, pattern = { type = "checks", color_a = { r = 0.25, g = 0.25, b = 0.25 },
                                                               color_b = { r = 0.75, g = 0.75, b = 0.75 }, scale = 1.5 } } },
      red, steel,
      { type = "cube", material = MATT, color = { r = 0.2, g = 0.5, b = 0.8 }, rotate_y = 0.5, scale = 0.6, position = { x = 0.2, y = 0.6, z = 2.2 } },
   },
}
math.randomseed(7)
for n = 1, BALLS do
   local s = 0.1 + 0.2 * math.random()
   table.insert(world.shapes, { type = "sphere", material = MATT, color = { r = math.random(), g = math.random(), b = math.random() }, scale = s,
                                position = { x = (2 * math.random() - 1) * 5, y = s, z = 1 + 5 * math.random() } })
end

camera = {
   screenwidth = WIDTH, screenheight = HEIGHT,
   position = { x = 0, y = 2.5, z = -8 },
   lookat = { x = 0, y = 1.2, z = 0 }, up = { x = 0, y = 1, z = 0 },
   fov = math.pi / 3,
}

local film = StartAnimation("bouncing.gif")
for frame = 0, FRAMES - 1 do
   local t = frame / FRAMES
   red.position.y = ball_height(t, 0.7, 2.5, 2)
   if not ONLY_RED then
      steel.position.y = ball_height(t, 0.5, 1.5, 3)
      world.lights[1].position.x = light_x(t)
   end
   print(string.format("frame %d: red %.6f steel %.6f light %.6f", frame, red.position.y, steel.position.y, world.lights[1].position.x))
   film:AddFrame(world, camera)
end
film:Finish()
print("frames: " .. FRAMES)
