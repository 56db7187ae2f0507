-- The Lua twin of soft_shadows.yml: a 4 x 4 area light (the keys corner, uvec, vvec, usteps, vsteps beside color; the
-- steps are Lua integers) and a dim point fill light over a floor, three spheres and a cube.
local lights = {
   { color = { r = 1.2, g = 1.15, b = 1.05 },
     corner = { x = -3, y = 6, z = -5 }, uvec = { x = 2, y = 0, z = 0 }, vvec = { x = 0, y = 0.5, z = 2 },
     usteps = 4, vsteps = 4 },
   { color = { r = 0.1, g = 0.13, b = 0.2 }, position = { x = 6, y = 1.5, z = -4 } },
}
local world = { lights = lights, shapes = {
   { type = "plane", material = { specular = 0, pattern = { type = "checks",
       color_a = { r = 0.4, g = 0.4, b = 0.4 }, color_b = { r = 0.7, g = 0.7, b = 0.7 } } } },
   { type = "sphere", position = { x = -1.5, y = 1, z = 0.5 }, color = { r = 0.85, g = 0.25, b = 0.2 },
     material = { diffuse = 0.7, specular = 0.6, shininess = 120.0 } },
   { type = "sphere", position = { x = 0.6, y = 0.6, z = -1.4 }, scale = 0.6, color = { r = 0.2, g = 0.35, b = 0.8 },
     material = { diffuse = 0.8, specular = 0.4 } },
   { type = "sphere", position = { x = -0.4, y = 0.35, z = -2.2 }, scale = 0.35, color = { r = 0.9, g = 0.8, b = 0.25 },
     material = { specular = 0.2 } },
   { type = "cube", position = { x = 2.3, y = 0.5, z = 1.2 }, scale = 0.5, rotate_y = 0.6, color = { r = 0.25, g = 0.6, b = 0.35 },
     material = { diffuse = 0.8, specular = 0.2 } },
} }
local camera = { screenwidth = 320, screenheight = 200, fov = 0.9,
                 position = { x = 0, y = 2.6, z = -7.5 }, lookat = { x = 0, y = 0.8, z = 0 }, up = { x = 0, y = 1, z = 0 } }
Render(world, camera, "soft_shadows.png")
